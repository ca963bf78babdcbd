"""tests/ckks_eval_mod_ref.py -- the definition the device is held to -- held to anchors that exist without it:

* the power rule (T_k from its halves: 2 T_a T_b - 1 or - T_1) and the Chebyshev split, walked in plain doubles, against
  numpy.polynomial.chebyshev.chebval for m = 2, 4, 8 and every degree 3 .. 63;
* the plans (he355_ckks_eval_chebyshev_plan, he355_ckks_eval_mod_plan: no device) against the brute-force walk of the definition in the
  reference, on a table of shapes;
* one even and one odd power step against the oracle's multiply_ntt / relinearize / combination / rescale spelled out;
* r = 0 gives the Chebyshev call's bits; the scales of the double angles arrive at out_scale up to rounding;
* accuracy with real keys at N = 2048, scale 2^40, chain {60, 40 x 7, 60}, (K = 3, r = 2, degree 15): the slot error against numpy's value
  of the same polynomial and double angles is held to 2 x the error of the yardstick -- the MONOMIAL tree on cheb2poly of the same
  coefficients and r double angles through the oracle's public calls, on the same ciphertext; the factor covers the rounded scalars of
  the power steps and the doubled product.  Loosely also against sin(2 pi v).  Measured figures: profiles/ckks_eval_mod.txt.
No GPU."""
import importlib
import math
import os

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

import ckks_eval_mod_ref as mref
import ckks_eval_poly_ref as ref
import oracle as ho

N = 2048
BITS8 = [60] + [40] * 7 + [60]
SCALE = 2.0 ** 40
K, R, DEGREE = 3, 2, 15
FACTOR = 2.0


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


def walk_in_doubles(c, m, u):
    """the definition's recursion on numbers: powers from their halves, leaves as sums, nodes through the Chebyshev split"""
    T = {0: np.ones_like(u), 1: u}

    def power(k):
        if k not in T:
            b, a = k // 2, k - k // 2
            T[k] = 2.0 * power(a) * power(b) - (T[0] if k % 2 == 0 else u)
        return T[k]

    def ev(p):
        deg = len(p) - 1
        if deg < m:
            return sum(p[k] * power(k) for k in range(deg + 1))
        e = m
        while 2 * e <= deg:
            e *= 2
        hi, lo = mref.cheb_split(p, e)
        out = (ev(hi) if len(hi) > 1 else hi[0]) * power(e)
        return out + ev(lo) if lo else out

    return ev(ref.trimmed(c))


@pytest.mark.parametrize("m", [2, 4, 8])
def test_the_power_rule_and_the_split_against_chebval(m):
    rng = np.random.default_rng(m)
    u = np.concatenate([np.linspace(-1.0, 1.0, 65), rng.uniform(-1, 1, 64)])
    for deg in range(3, 64):
        c = rng.uniform(-1.0, 1.0, deg + 1)
        if deg % 5 == 0:
            c[::2] = 0.0  # odd only
            c[-1] = 0.7
        got, want = walk_in_doubles(list(c), m, u), cheb.chebval(u, c)
        assert np.max(np.abs(got - want)) < 1e-11 * (deg + 1), (m, deg)


def dense(deg):
    return [0.3 + 0.01 * k for k in range(deg + 1)]


SHAPES = ([(f"dense {d}", dense(d)) for d in (1, 2, 3, 7, 8, 15, 31)]
          + [("odd 7", [0.0 if k % 2 == 0 else 0.1 * k for k in range(8)]), ("odd 15", [0.0 if k % 2 == 0 else 0.1 * k for k in range(16)]),
             ("even 14", [0.2 if k % 2 == 0 else 0.0 for k in range(15)]), ("T_15", [0.0] * 15 + [1.0]), ("T_8", [0.0] * 8 + [0.5]),
             ("1 + T_8", [1.0] + [0.0] * 7 + [0.5]), ("T_1 + T_12", [0.0, 1.0] + [0.0] * 10 + [2.0]), ("cancelling low", [0.5, 0.0, 0.25, 0.0, 0.0, 0.0, 0.25]),
             ("eval mod 3 2 15", mref.eval_mod_coeffs(3, 2, 15))])
KEYS = ("depth", "L_out", "degree", "products", "combinations", "rescales", "drops", "adds", "powers", "min_scalar_bits")


@pytest.mark.parametrize("log_baby", [1, 2, 3])
@pytest.mark.parametrize("name,coeffs", SHAPES, ids=[s[0] for s in SHAPES])
def test_the_plans_against_the_brute_force_walk(be, name, coeffs, log_baby):
    bits = [60] + [40] * 8 + [60]
    o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    assert [int(be.lib().he355_modulus(g.h, i)) for i in range(g.L)] == o.moduli[:o.L]
    L = o.L
    ev = mref.Evaluator(o, coeffs, log_baby, L, SCALE, SCALE)
    ev.count()
    want = ev.counters()
    pl = g.ckks_eval_chebyshev_plan(L, coeffs, log_baby, SCALE, SCALE)
    assert {k: pl[k] for k in KEYS} == want
    assert pl["powers_computed"] == ev.powers and pl["double_angles"] == 0 and pl["out_scale"] == SCALE
    for r in (0, 1, 3):
        if want["depth"] + r >= L:
            with pytest.raises(be.HE355Error, match="he355_ckks_eval_mod_plan"):
                g.ckks_eval_mod_plan(L, coeffs, log_baby, SCALE, SCALE, r)
            continue
        mv = mref.ModEvaluator(o, coeffs, log_baby, L, SCALE, SCALE, r)
        mv.count()
        wm = mv.counters()
        pm = g.ckks_eval_mod_plan(L, coeffs, log_baby, SCALE, SCALE, r)
        assert {k: pm[k] for k in KEYS + ("double_angles",)} == wm, r
        assert pm["out_scale"] == mv.out_scale and abs(pm["out_scale"] / SCALE - 1.0) < 1e-12
    g.close()


@pytest.fixture(scope="module")
def keyed():
    o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=BITS8, sec128=False)
    sk = o.keygen_secret(300)
    return o, sk, o.keygen_public(sk, 301), o.keygen_relin(sk, 302)


def test_a_power_step_against_the_oracles_own_calls(keyed):
    o, sk, pk, rk = keyed
    rng = np.random.default_rng(5)
    L, q = o.L, o.moduli
    x = o.encrypt(pk, ho.ckks_encode(o, rng.uniform(-1, 1, N // 2), SCALE), 303)
    out, ev = mref.eval_chebyshev(o, x, [0.0, 0.0, 0.0, 1.0], 2, SCALE, SCALE, rk)
    assert ev.powers == [2, 3] and (ev.products, ev.rescales, ev.combinations, ev.drops, ev.adds) == (2, 3, 0, 1, 0)
    W2 = SCALE * SCALE
    P2 = o.relinearize(o.multiply_ntt(x, x), rk)
    T2 = o.rescale(ref.combine_composed(o, L, [P2], [[2] * L], ref.scalar_residues(q, L, -W2)))
    assert np.array_equal(ev.val[2], T2)
    s2 = W2 / float(q[L - 1])
    assert ev.scale[2] == s2 and ev.level[2] == L - 1
    W3 = s2 * SCALE
    P3 = o.relinearize(o.multiply_ntt(T2, o.mod_switch_drop(x, L - 1)), rk)
    T3 = o.rescale(ref.combine_composed(o, L - 1, [P3, x], [[2] * (L - 1), ref.scalar_residues(q, L - 1, -(W3 / SCALE))]))
    assert np.array_equal(ev.val[3], T3)
    # T_3 = 4 u^3 - 3 u in the slots
    u = ho.ckks_decode(o, o.decrypt_phase(x, sk), SCALE).real
    got = ho.ckks_decode(o, o.decrypt_phase(ev.val[3], sk), ev.scale[3]).real
    assert np.max(np.abs(got - (4 * u ** 3 - 3 * u))) < 1e-6


def test_no_double_angle_is_the_chebyshev_call(keyed):
    o, sk, pk, rk = keyed
    rng = np.random.default_rng(6)
    x = o.encrypt(pk, ho.ckks_encode(o, rng.uniform(-1, 1, N // 2), SCALE), 304)
    c = [0.1, -0.4, 0.3, 0.0, 0.25]
    a, _ = mref.eval_chebyshev(o, x, c, 1, SCALE, SCALE, rk, composed=True)
    b, mv = mref.eval_mod(o, x, c, 1, SCALE, SCALE, 0, rk, composed=True)
    assert np.array_equal(a, b) and mv.out_scale == SCALE


def slot_error(o, sk, ct, scale, want):
    got = ho.ckks_decode(o, o.decrypt_phase(ct, sk), scale)
    return float(np.max(np.abs(got.real - want)))


def eval_mod_case(o, pk, seed):
    """(u, v = K u within 2^-8 of integers below K, the ciphertext of u, numpy's value of the polynomial and double angles)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-(K - 1), K, N // 2) + rng.uniform(-2.0 ** -8, 2.0 ** -8, N // 2)
    u = v / K
    c = mref.eval_mod_coeffs(K, R, DEGREE)
    return u, v, c, o.encrypt(pk, ho.ckks_encode(o, u, SCALE), seed + 1), mref.double_angles(cheb.chebval(u, c), R)


def test_accuracy_of_eval_mod_against_the_monomial_yardstick(keyed):
    o, sk, pk, rk = keyed
    u, v, c, x, want = eval_mod_case(o, pk, 400)
    out, mv = mref.eval_mod(o, x, c, 1, SCALE, SCALE, R, rk, composed=True)
    assert out.shape == (2, o.L - 4 - R, N)
    yard, ys = mref.yardstick(o, x, c, 1, SCALE, SCALE, R, rk)
    e_new, e_yard = slot_error(o, sk, out, mv.out_scale, want), slot_error(o, sk, yard, ys, want)
    e_sin = slot_error(o, sk, out, mv.out_scale, np.sin(2.0 * math.pi * v))
    print(f"eval mod (K {K}, r {R}, degree {DEGREE}) on {BITS8}: chebyshev {e_new:.3e}  monomial yardstick {e_yard:.3e}  ratio {e_new / e_yard:.2f}  "
          f"against sin(2 pi v): {e_sin:.3e}")
    assert e_yard < 1e-3  # (the yardstick itself works)
    assert e_new <= FACTOR * e_yard
    assert e_sin < 1e-3  # loosely: the interpolation error in doubles is 6.3e-7
