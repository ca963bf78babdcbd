"""tests/ckks_mod_raise_ref.py -- the definition of he355_ckks_mod_raise the device is held to -- against exact integers at N = 1024, on
{60, 40, 40, 60}, {40, 60, 60}, {42, 38, 45, 44} and the `tiny_n1024` chain of tests/explicit_moduli.py (a 60-bit prime 0 over 14-bit moduli):

* CRT-composing the raised polynomial over Q_to = q_0 .. q_{L_to - 1} gives exactly the centred c, for every L_to (for a Q_to below q_0: c mod Q_to, centred);
* row 0 of the output is the input's row 0; rows >= 1 of the input do not matter;
* the tie points (q_0 - 1) / 2 and (q_0 + 1) / 2 land on opposite signs: +(q_0 - 1) / 2 and -(q_0 - 1) / 2;
* the decryption identity: a hand-made symmetric ciphertext under q_0 (c_1 uniform, c_0 = -c_1 s + m + e, s ternary of Hamming weight
  h = 16, never uploaded anywhere) raised to L_top and decrypted in Python over Q_to equals m' + q_0 I, m' the centred level-1 decryption:
  every coefficient of the difference is divisible by q_0 and |I| <= (h + 2) / 2 = 9.  The bound: |c_0 + c_1 s| <= (q_0 - 1)(1 + h) / 2 over the
  integers (centred c_0, c_1; s has h entries of +-1), and |m'| <= (q_0 - 1) / 2, so |q_0 I| <= (q_0 - 1)(h + 2) / 2.
No GPU."""
import numpy as np
import pytest

import ckks_mod_raise_ref as ref
import explicit_moduli as em

N = 1024
CHAINS = {"60_40_40_60": [60, 40, 40, 60], "40_60_60": [40, 60, 60], "42_38_45_44": [42, 38, 45, 44], "tiny_n1024": None}
H = 16


@pytest.fixture(scope="module", params=list(CHAINS))
def ctx(request, oracle):
    bits = CHAINS[request.param]
    if bits is None:
        o = oracle.Context(oracle.SCHEME_CKKS, N, primes=em.load()[request.param]["primes"])
    else:
        o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    L = len(o.moduli) - 1
    return o, [int(q) for q in o.moduli[:L]], np.random.default_rng(len(request.param))


def crt_centred(rows, moduli):
    """rows [L][N] residues (coefficient form) -> [N] Python integers in (-Q / 2, Q / 2]"""
    Q = 1
    for q in moduli:
        Q *= q
    acc = np.zeros(rows.shape[-1], dtype=object)
    for r, q in zip(rows, moduli):
        Qi = Q // q
        acc = (acc + r.astype(object) * (Qi * pow(Qi, -1, q))) % Q
    return np.where(acc > Q // 2, acc - Q, acc), Q


def coefficients(o, x):
    return np.stack([o.intt(i, np.ascontiguousarray(x[i])) for i in range(x.shape[0])])


def negacyclic(a, s):
    """a [N] integers times the sparse ternary s [N] in Z[X] / (X^N + 1), exact"""
    n = len(a)
    out = np.zeros(n, dtype=object)
    for k in np.nonzero(s)[0]:
        rolled = np.concatenate([-a[n - k:], a[:n - k]]) if k else a
        out = out + int(s[k]) * rolled
    return out


def test_crt_of_the_raise_is_the_centred_integer(ctx):
    o, q, rng = ctx
    Lt = len(q)
    pats = ref.patterns(q, N, rng)
    for name, coeff in pats.items():
        c = ref.centred(coeff, q[0])
        x = np.stack([o.ntt(0, coeff)] + [rng.integers(0, q[i], N, dtype=np.uint64) for i in range(1, Lt)])  # rows >= 1: garbage
        for L_to in range(1, Lt + 1):
            out = ref.mod_raise(o, x, L_to)
            assert out.shape == (L_to, N)
            assert np.array_equal(out[0], x[0]), (name, "row 0")
            assert np.array_equal(out, ref.mod_raise(o, x[:1], L_to)), (name, "rows >= 1 of the input matter")
            got, Q = crt_centred(coefficients(o, out), q[:L_to])
            if Q > q[0]:
                assert (got == c).all(), (name, L_to)
            else:
                want = c % Q
                assert (got == np.where(want > Q // 2, want - Q, want)).all(), (name, L_to)
            assert np.array_equal(coefficients(o, out), ref.lift_centred(q, coeff, L_to)), (name, L_to, "the lift on its own")


def test_the_tie_points_land_on_opposite_signs(ctx):
    o, q, rng = ctx
    half = (q[0] - 1) // 2
    assert ref.centred([half, half + 1], q[0]).tolist() == [half, -half]
    coeff = np.zeros(N, dtype=np.uint64)
    coeff[0], coeff[1] = half, half + 1
    out = ref.mod_raise(o, np.stack([o.ntt(0, coeff)]), len(q))
    got, Q = crt_centred(coefficients(o, out), q)
    assert Q > q[0] and got[0] == half and got[1] == -half and not got[2:].any()
    for j in range(1, len(q)):
        cj = coefficients(o, out)[j]
        assert int(cj[0]) == half % q[j] and int(cj[1]) == (-half) % q[j]


def test_the_decryption_identity(ctx):
    o, q, rng = ctx
    q0, Lt = q[0], len(q)
    s = np.zeros(N, dtype=np.int64)
    s[rng.choice(N, H, replace=False)] = rng.choice([-1, 1], H)
    assert np.count_nonzero(s) == H
    c1 = rng.integers(0, q0, N, dtype=np.uint64).astype(object)
    m = rng.integers(-(1 << 20), 1 << 20, N).astype(object)
    e = rng.integers(-8, 9, N).astype(object)
    c0 = (m + e - negacyclic(c1, s)) % q0
    ct = np.stack([np.stack([o.ntt(0, np.array(c, dtype=np.uint64))]) for c in (c0, c1)])  # [2][1][N], NTT form under q_0
    low = (c0 + negacyclic(c1, s)) % q0
    m1 = np.where(low > (q0 - 1) // 2, low - q0, low)  # the level-1 decryption, centred
    assert (m1 == m + e).all()
    up = ref.mod_raise(o, ct, Lt)  # [2][Lt][N]
    rows = []
    for j in range(Lt):  # decrypt under every prime of Q_to: c_0 + c_1 s mod q_j
        a0, a1 = (o.intt(j, np.ascontiguousarray(up[k, j])).astype(object) for k in range(2))
        rows.append(((a0 + negacyclic(a1, s)) % q[j]).astype(object))
    dec, Q = crt_centred(np.stack(rows), q)
    assert Q > q0 * (H + 2)  # the integers below fit Q: the identity is over Z
    diff = dec - m1
    assert not (diff % q0).any()
    I = diff // q0
    assert int(np.max(np.abs(I))) <= (H + 2) // 2 == 9
    assert I.any()  # the raise does add multiples of q_0: that is what the circuit removes
