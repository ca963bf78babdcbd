"""The definition of the lazy-mod-down plain sum (tests/rotate_hoisted_lazy_ref.py: Python integers and the oracle's transforms) on the CPU:

* its bit-exact anchors in the oracle.  P is odd, so centring commutes with the signed coefficient permutation and the mod-down commutes with
  sigma: a sum of ONE keyed step whose plaintext is the all-ones NTT vector on all L + 1 rows equals rotate_hoisted_ref.hoisted bit for bit, and
  a sum of identity steps only equals multiply_plain + add -- CKKS N = 1024 {50,40,40,50} at L = 3 and 2, N = 2048 {45,52} at L = 1, BFV
  N = 1024 {50,40,40,50} in NTT form at L = 3 and 2;
* the five-term sum [0, 1, -2, 3, 1] differs from rotate_hoisted_ref.plain_sum (a sum of mod-downs is not the mod-down of the sum) yet decrypts
  like it under real keys: CKKS N = 1024 with a 16-diagonal matrix at scale 2^30 -- the slot error within rotate_hoisted_ref.CKKS_ERROR_CAP x the
  eager sum's on the same inputs, both printed -- and BFV N = 2048 {60,40,60}, t of 20 bits: the decoded product exact, both noise budgets
  (from decrypt_phase) printed;
* extend_special against direct reduction of the integer coefficients, and a planted plaintext with a coefficient of floor(q_0 / 2) + 5: a
  non-zero mismatch count at L >= 2, zero at L = 1.
No GPU, no backend."""
import numpy as np
import pytest

import rotate_hoisted_lazy_ref as lazy
import rotate_hoisted_ref as ref

CONTEXTS = {
    "ckks1024": ("CKKS", 1024, [50, 40, 40, 50]),
    "ckks2048": ("CKKS", 2048, [45, 52]),
    "bfv1024": ("BFV", 1024, [50, 40, 40, 50]),
}
STEPS = [0, 1, -2, 3, 1]


def make(oracle, name):
    scheme, N, bits = CONTEXTS[name]
    if scheme == "CKKS":
        return oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    return oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)


def levels(o):
    return [o.L] + ([o.L - 1] if o.L > 1 else [])


def random_plain_qp(o, rng, L, count):
    return np.stack([o.random_poly(rng, L, 1, special=True)[0] for _ in range(count)])


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_the_two_anchors_in_the_oracle(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(len(name) + o.N)
    for L in levels(o):
        ct = o.random_poly(rng, L, 2)
        for s in (1, -2):
            g = o.galois_elt(s)
            key = o.random_kswitch_key(rng)
            got = lazy.plain_sum_lazy(o, ct[None], [s], {g: key}, lazy.ones_qp(o, L)[None])[0]
            assert np.array_equal(got, ref.hoisted(o, ct, g, key, 1)), (name, L, s)
        plains = random_plain_qp(o, rng, L, 3)
        got = lazy.plain_sum_lazy(o, ct[None], [0, 0, 0], {}, plains)[0]
        want = None
        for p in plains:
            t = o.multiply_plain(ct, p[:L])
            want = t if want is None else o.add(want, t)
        assert np.array_equal(got, want), (name, L)


@pytest.mark.parametrize("name", ["ckks1024", "bfv1024"])
def test_the_general_sum_is_not_the_eager_sums_bits(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(5 + o.N)
    L = o.L
    keys = {o.galois_elt(s): o.random_kswitch_key(rng) for s in set(STEPS) if s}
    ct = o.random_poly(rng, L, 2)
    plains = random_plain_qp(o, rng, L, len(STEPS))
    got = lazy.plain_sum_lazy(o, ct[None], STEPS, keys, plains)[0]
    assert not np.array_equal(got, ref.plain_sum(o, ct[None], STEPS, keys, plains[:, :L])[0])
    # the order of the terms does not matter
    order = [3, 0, 4, 2, 1]
    again = lazy.plain_sum_lazy(o, ct[None], [STEPS[i] for i in order], keys, plains[order])[0]
    assert np.array_equal(got, again)


def _diagonals(n, count, diags):
    M = np.zeros((n, n), dtype=diags.dtype)
    for s in range(count):
        M[np.arange(n), (np.arange(n) + s) % n] = diags[s]
    return M


def test_ckks_real_keys_sixteen_diagonals(oracle):
    N, bits = 1024, [50, 40, 40, 50]
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    L, n, scale = o.L, N // 2, 2.0 ** 30
    sk = o.keygen_secret(11)
    pk = o.keygen_public(sk, 12)
    steps = list(range(16))
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), 100 + s) for s in steps[1:]}
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    diags = rng.uniform(-1, 1, (16, n))
    want = _diagonals(n, 16, diags) @ x
    ct = o.encrypt(pk, oracle.ckks_encode(o, x, scale), 21)
    plains = np.stack([oracle.ckks_encode(o, d, scale) for d in diags])
    ext = [lazy.extend_special(o, p) for p in plains]
    assert all(bad == 0 for _, bad in ext)
    plain_qp = np.stack([e for e, _ in ext])
    got = lazy.plain_sum_lazy(o, ct[None], steps, keys, plain_qp)[0]
    eager = ref.plain_sum(o, ct[None], steps, keys, plains)[0]
    assert not np.array_equal(got, eager)
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    err_l, err_e = np.abs(dec(got) - want).max(), np.abs(dec(eager) - want).max()
    print(f"16 diagonals: eager {err_e:.3e} lazy {err_l:.3e}")
    assert err_e < 1e-2, err_e
    assert err_l <= ref.CKKS_ERROR_CAP * err_e, (err_l, err_e)


def bfv_budget(o, ct_ntt, sk):
    """the invariant noise budget of an NTT-form ciphertext from decrypt_phase: log2(q / (2 |t phase mod q|)) bits, the residue centred"""
    L = ct_ntt.shape[1]
    ct = np.stack([np.stack([o.intt(i, ct_ntt[k, i]) for i in range(L)]) for k in range(2)])
    phase = o.decrypt_phase(ct, sk)  # [L][N] coefficient form
    q = 1
    for m in o.moduli[:L]:
        q *= m
    x = np.zeros(o.N, dtype=object)
    for i, m in enumerate(o.moduli[:L]):  # CRT
        qi = q // m
        x = (x + phase[i].astype(object) * (pow(qi, -1, m) * qi)) % q
    v = (x * o.t) % q
    v = np.where(v > q // 2, q - v, v)
    worst = int(max(v.max(), 1))
    return q.bit_length() - worst.bit_length() - 1


def test_bfv_real_keys_five_terms(oracle):
    N, bits = 2048, [60, 40, 60]
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L, half, t = o.L, N // 2, o.t
    codec = oracle.BatchCodec(N, t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), 200 + s) for s in set(STEPS) if s}
    rng = np.random.default_rng(6)
    x = rng.integers(0, t, N)
    diags = rng.integers(0, t, (len(STEPS), N))
    ct = o.encrypt(pk, codec.encode(x), 41)
    ct_ntt = np.stack([np.stack([o.ntt(i, ct[k, i]) for i in range(L)]) for k in range(2)])
    plains = []
    for d in diags:  # the centred lift of a plaintext mod t, NTT form: what he355_bfv_plain_to_ntt makes
        m = codec.encode(d).astype(object)
        m = np.where(m > t // 2, m - t, m)
        plains.append(np.stack([o.ntt(i, (m % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])]))
    plains = np.stack(plains)
    ext = [lazy.extend_special(o, p) for p in plains]
    assert all(bad == 0 for _, bad in ext)
    plain_qp = np.stack([e for e, _ in ext])
    got = lazy.plain_sum_lazy(o, ct_ntt[None], STEPS, keys, plain_qp)[0]
    eager = ref.plain_sum(o, ct_ntt[None], STEPS, keys, plains)[0]
    assert not np.array_equal(got, eager)
    want = np.zeros(N, dtype=object)
    for s, d in zip(STEPS, diags):
        for lo in (0, half):
            want[lo:lo + half] += d[lo:lo + half].astype(object) * np.roll(x[lo:lo + half], -s).astype(object)
    want %= t
    back = lambda c: np.stack([np.stack([o.intt(i, c[k, i]) for i in range(L)]) for k in range(2)])
    for name, c in (("lazy", got), ("eager", eager)):
        dec = codec.decode(o.bfv_decode_phase(o.decrypt_phase(back(c), sk)))
        assert np.array_equal(dec.astype(object) % t, want), name
    b_l, b_e = bfv_budget(o, got, sk), bfv_budget(o, eager, sk)
    print(f"noise budget: eager {b_e} lazy {b_l} bits")
    assert b_l > 0 and b_e > 0


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_extend_special_is_the_reduction_of_the_integer_coefficients(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(o.N + 3)
    P, q0 = o.moduli[o.K - 1], o.moduli[0]
    for L in levels(o):
        lim = min(q0 // 2, 1 << 40)
        c = rng.integers(-lim, lim + 1, o.N).astype(object)
        c[0], c[1], c[2] = q0 // 2, -(q0 // 2), 0  # the ends of (-q_0 / 2, q_0 / 2]
        plain = np.stack([o.ntt(i, (c % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])])
        got, bad = lazy.extend_special(o, plain)
        assert bad == 0 and np.array_equal(got[:L], plain)
        assert np.array_equal(got[L], o.ntt(o.K - 1, (c % P).astype(np.uint64))), (name, L)
        # a planted coefficient of floor(q_0 / 2) + 5: prime 0 reads it as negative, the other primes do not agree
        c[7] = q0 // 2 + 5
        planted = np.stack([o.ntt(i, (c % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])])
        _, bad = lazy.extend_special(o, planted)
        assert (bad > 0) == (L >= 2), (name, L, bad)
        assert bad == (L - 1 if L >= 2 else 0), (name, L, bad)
