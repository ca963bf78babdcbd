"""The hoisted rotation's definition (tests/rotate_hoisted_ref.py, the composition of oracle calls the device is held to bit for bit) is a
rotation: with real keys from the oracle's key generator at N = 1024, {50, 40, 40, 50},

* BFV (t of 20 bits), steps 1, 7, -2 and element 2N - 1: it decrypts to EXACTLY the plaintext the ordinary rotation decrypts to;
* CKKS (scale 2^30), steps 1, 5, -3 and the conjugation, at L_top and L_top - 1: the slot error is at most CAP = 2 x the ordinary rotation's on
  the same ciphertext (measured: 1.46 x at the most; a wrong key permutation or element gives errors of the size of the values, 10^4 x);
* the bits differ from apply_galois (the definition is the library's own), in every case;
* c1 = 0 gives exactly (sigma(c0), 0);
* the plain sum over the diagonals of a cyclic-diagonal matrix decodes to numpy's matrix-vector product, within CAP x the error of the same
  sum over ordinary rotations.
No GPU, no backend."""
import numpy as np
import pytest

import rotate_hoisted_ref as ref

N, BITS = 1024, [50, 40, 40, 50]
CAP = ref.CKKS_ERROR_CAP


@pytest.fixture(scope="module")
def ckks(oracle):
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=BITS, sec128=False)
    sk = o.keygen_secret(11)
    pk = o.keygen_public(sk, 12)
    scale = 2.0 ** 30
    x = np.random.default_rng(7).uniform(-1, 1, N // 2)
    ct = o.encrypt(pk, oracle.ckks_encode(o, x, scale), 21)
    elts = {s: o.galois_elt(s) for s in (1, 5, -3)}
    elts["conj"] = 2 * N - 1
    keys = {e: o.keygen_galois(sk, e, 100 + i) for i, e in enumerate(elts.values())}
    return dict(o=o, sk=sk, scale=scale, x=x, ct=ct, elts=elts, keys=keys)


def _slots(oracle, e, ct, scale=None):
    return oracle.ckks_decode(e["o"], e["o"].decrypt_phase(ct, e["sk"]), scale or e["scale"])


def _want(x, s):
    return np.conj(x) if s == "conj" else np.roll(x, -s)


@pytest.mark.parametrize("drop", [0, 1])
def test_ckks_error_within_twice_the_ordinary_rotation(oracle, ckks, drop):
    e, o = ckks, ckks["o"]
    ct = o.mod_switch_drop(e["ct"], o.L - drop)
    for s, g in e["elts"].items():
        ordinary = o.apply_galois(ct, g, e["keys"][g])
        got = ref.hoisted(o, ct, g, e["keys"][g])
        assert not np.array_equal(got, ordinary), s
        want = _want(e["x"], s)
        err_o = np.abs(_slots(oracle, e, ordinary) - want).max()
        err_h = np.abs(_slots(oracle, e, got) - want).max()
        print(f"L {o.L - drop} step {s}: ordinary {err_o:.3e} hoisted {err_h:.3e} ratio {err_h / err_o:.3f}")
        assert err_o < 1e-3, (s, err_o)  # the ordinary rotation is that rotation
        assert err_h <= CAP * err_o, (s, err_h, err_o)


def test_ckks_c1_zero_is_the_permutation_alone(ckks):
    e, o = ckks, ckks["o"]
    ct = e["ct"].copy()
    ct[1] = 0
    for g in e["elts"].values():
        got = ref.hoisted(o, ct, g, e["keys"][g])
        assert not got[1].any()
        assert np.array_equal(got[0], np.stack([o.apply_galois_poly(i, g, 1, ct[0, i]) for i in range(o.L)]))
    assert np.array_equal(ref.hoisted(o, e["ct"], 1, None), e["ct"])  # the identity needs no key


def test_ckks_plain_sum_is_the_matrix_vector_product(oracle, ckks):
    e, o = ckks, ckks["o"]
    n, steps = N // 2, [0, 1, 5, -3]
    rng = np.random.default_rng(8)
    diags = rng.uniform(-1, 1, (len(steps), n))
    M = np.zeros((n, n))
    for d, s in zip(diags, steps):
        M[np.arange(n), (np.arange(n) + s) % n] = d
    want = M @ e["x"]
    plains = np.stack([oracle.ckks_encode(o, d, e["scale"]) for d in diags])
    keys = {o.galois_elt(s): e["keys"][o.galois_elt(s)] for s in steps if s}
    got = ref.plain_sum(o, e["ct"][None], steps, keys, plains)[0]
    acc = None
    for s, p in zip(steps, plains):
        t = o.multiply_plain(e["ct"] if s == 0 else o.apply_galois(e["ct"], o.galois_elt(s), keys[o.galois_elt(s)]), p)
        acc = t if acc is None else o.add(acc, t)
    err_h = np.abs(_slots(oracle, e, got, e["scale"] ** 2) - want).max()
    err_o = np.abs(_slots(oracle, e, acc, e["scale"] ** 2) - want).max()
    print(f"plain sum: ordinary {err_o:.3e} hoisted {err_h:.3e}")
    assert err_o < 1e-3 and err_h <= CAP * err_o, (err_h, err_o)


def test_bfv_decrypts_to_the_ordinary_rotation_exactly(oracle):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=BITS, plain_bits=20, sec128=False)
    codec = oracle.BatchCodec(N, o.t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    x = np.random.default_rng(9).integers(0, o.t, N)
    ct = o.encrypt(pk, codec.encode(x), 41)
    dec = lambda c: codec.decode(o.bfv_decode_phase(o.decrypt_phase(c, sk)))
    for i, g in enumerate([o.galois_elt(1), o.galois_elt(7), o.galois_elt(-2), 2 * N - 1]):
        key = o.keygen_galois(sk, g, 200 + i)
        ordinary = o.apply_galois(ct, g, key)
        got = ref.hoisted(o, ct, g, key)
        assert not np.array_equal(got, ordinary), g
        d = dec(ordinary)
        assert not np.array_equal(d, dec(ct)) and sorted(d) == sorted(dec(ct)), g  # a rotation of the rows (or their swap)
        assert np.array_equal(dec(got), d), g
        # NTT-form BFV ciphertexts: the same ciphertext, transformed
        ntt = np.stack([np.stack([o.ntt(j, ct[k, j]) for j in range(o.L)]) for k in range(2)])
        back = ref.hoisted(o, ntt, g, key, ntt_form=1)
        assert np.array_equal(np.stack([np.stack([o.intt(j, back[k, j]) for j in range(o.L)]) for k in range(2)]), got), g
    z = ct.copy()
    z[1] = 0
    g = o.galois_elt(1)
    got = ref.hoisted(o, z, g, o.keygen_galois(sk, g, 200))
    assert not got[1].any() and np.array_equal(got[0], np.stack([o.apply_galois_poly(i, g, 0, z[0, i]) for i in range(o.L)]))
