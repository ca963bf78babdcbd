"""The definition of the baby-step/giant-step linear transform (tests/linear_transform_bsgs_ref.py) on the CPU, against what already exists,
bit for bit:

* one identity giant row: rotate_hoisted_lazy_ref.plain_sum_lazy over the baby steps (mod_down(A + P B) = B + mod_down(A));
* one identity baby with all-ones plaintexts: plain_sum_lazy over the giant steps with ones_qp (mod_down(P X) = X);
* all steps the identity: multiply_plain + add;
* a mask: the same call with the masked terms' plaintexts zeroed -- and the masked column's key is not even given.
With real keys from the oracle (the ring of tests/test_rotate_hoisted_lazy_ref_cpu.py's real-key cases): a 16-diagonal cyclic matrix split
4 x 4 with pre-rotated diagonals -- BFV decrypts to M v mod t exactly; CKKS decodes to M v with a maximum slot error of at most 2 x the flat
lazy reference's over the same 16 steps on the same inputs.  Measured: BSGS 4.112e-05 against flat 3.493e-05, ratio 1.177
(profiles/linear_transform_bsgs.txt).
No GPU, no backend."""
import numpy as np
import pytest

import linear_transform_bsgs_ref as bsgs
import rotate_hoisted_lazy_ref as lazy
from test_rotate_hoisted_lazy_ref_cpu import CONTEXTS, _diagonals, levels, make, random_plain_qp

BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
CKKS_RATIO_CAP = 2.0  # the giant key switch's noise is not multiplied by a plaintext: a ratio near 1; the hoisted calls' seed-to-seed spread is 0.33 - 1.46


def rand_keys(o, rng, steps):
    return {o.galois_elt(s): o.random_kswitch_key(rng) for s in set(steps) if s}


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_one_identity_giant_row_is_the_lazy_plain_sum(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(11 + o.N)
    baby = [0, 1, -2, 3, 1]
    keys = rand_keys(o, rng, baby)
    for L in levels(o):
        ct = o.random_poly(rng, L, 2)
        plains = random_plain_qp(o, rng, L, len(baby))
        got = bsgs.linear_transform_bsgs(o, ct[None], baby, [0], keys, plains[None])[0]
        assert np.array_equal(got, lazy.plain_sum_lazy(o, ct[None], baby, keys, plains)[0]), (name, L)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_one_identity_baby_with_ones_is_the_lazy_plain_sum_over_the_giants(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(12 + o.N)
    giant = [3, 0, -2]
    keys = rand_keys(o, rng, giant)
    for L in levels(o):
        ct = o.random_poly(rng, L, 2)
        ones = np.stack([lazy.ones_qp(o, L)] * len(giant))
        got = bsgs.linear_transform_bsgs(o, ct[None], [0], giant, keys, ones[:, None])[0]
        assert np.array_equal(got, lazy.plain_sum_lazy(o, ct[None], giant, keys, ones)[0]), (name, L)


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_identities_are_multiply_plain_and_add(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(13 + o.N)
    for L in levels(o):
        ct = o.random_poly(rng, L, 2)
        plains = random_plain_qp(o, rng, L, 6).reshape(2, 3, L + 1, o.N)
        got = bsgs.linear_transform_bsgs(o, ct[None], [0, 0, 0], [0, 0], {}, plains)[0]
        want = None
        for p in plains.reshape(6, L + 1, o.N):
            t = o.multiply_plain(ct, p[:L])
            want = t if want is None else o.add(want, t)
        assert np.array_equal(got, want), (name, L)


@pytest.mark.parametrize("name", ["ckks1024", "bfv1024"])
def test_a_mask_is_zeroed_plaintexts(oracle, name):
    o = make(oracle, name)
    rng = np.random.default_rng(14 + o.N)
    L = o.L
    baby, giant = [0, 1, -2], [0, 3]
    keys = rand_keys(o, rng, baby + giant)
    ct = o.random_poly(rng, L, 2)
    plains = random_plain_qp(o, rng, L, 6).reshape(2, 3, L + 1, o.N)
    for mask in ([[1, 0, 1], [1, 1, 1]], [[0, 0, 0], [1, 1, 0]], [[1, 0, 1], [0, 0, 1]]):
        zeroed = plains.copy()
        zeroed[~np.asarray(mask, dtype=bool)] = 0
        want = bsgs.linear_transform_bsgs(o, ct[None], baby, giant, keys, zeroed)[0]
        # a step whose every term is masked needs no key
        m = np.asarray(mask, dtype=bool)
        needed = {o.galois_elt(s) for i, s in enumerate(baby) if s and m[:, i].any()} | {o.galois_elt(s) for j, s in enumerate(giant) if s and m[j].any()}
        got = bsgs.linear_transform_bsgs(o, ct[None], baby, giant, {e: keys[e] for e in needed}, plains, mask)[0]
        assert np.array_equal(got, want), (name, mask)


def test_ckks_real_keys_sixteen_diagonals_four_by_four(oracle):
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

    def extended(v):
        e, bad = lazy.extend_special(o, oracle.ckks_encode(o, v, scale))
        assert bad == 0
        return e

    flat_qp = np.stack([extended(d) for d in diags])
    split = bsgs.split_diagonals(diags, BABY, GIANT, lambda v, s: np.roll(v, -s))
    plain_qp = np.stack([np.stack([extended(v) for v in row]) for row in split])
    got = bsgs.linear_transform_bsgs(o, ct[None], BABY, GIANT, keys, plain_qp)[0]
    flat = lazy.plain_sum_lazy(o, ct[None], steps, keys, flat_qp)[0]
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    err_b, err_f = np.abs(dec(got) - want).max(), np.abs(dec(flat) - want).max()
    print(f"16 diagonals: flat lazy {err_f:.3e} bsgs 4x4 {err_b:.3e} ratio {err_b / err_f:.3f}")
    assert err_f < 1e-2, err_f
    assert err_b <= CKKS_RATIO_CAP * err_f, (err_b, err_f)


def test_bfv_real_keys_sixteen_diagonals_four_by_four(oracle):
    N, bits = 2048, [60, 40, 60]
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L, half, t = o.L, N // 2, o.t
    codec = oracle.BatchCodec(N, t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), 200 + s) for s in set(BABY + GIANT) if s}
    rng = np.random.default_rng(6)
    x = rng.integers(0, t, N)
    diags = rng.integers(0, t, (16, N))
    ct = o.encrypt(pk, codec.encode(x), 41)
    ct_ntt = np.stack([np.stack([o.ntt(i, ct[k, i]) for i in range(L)]) for k in range(2)])
    rot = lambda v, s: np.concatenate([np.roll(v[:half], -s), np.roll(v[half:], -s)])  # both rows of the batching matrix rotate together

    def extended(v):  # the centred lift of a plaintext mod t, NTT form (what he355_bfv_plain_to_ntt makes), then the special row
        m = codec.encode(v).astype(object)
        m = np.where(m > t // 2, m - t, m)
        e, bad = lazy.extend_special(o, np.stack([o.ntt(i, (m % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])]))
        assert bad == 0
        return e

    plain_qp = np.stack([np.stack([extended(v) for v in row]) for row in bsgs.split_diagonals(diags, BABY, GIANT, rot)])
    got = bsgs.linear_transform_bsgs(o, ct_ntt[None], BABY, GIANT, keys, plain_qp)[0]
    want = np.zeros(N, dtype=object)
    for s in range(16):
        want += diags[s].astype(object) * rot(x, s).astype(object)
    back = np.stack([np.stack([o.intt(i, got[k, i]) for i in range(L)]) for k in range(2)])
    dec = codec.decode(o.bfv_decode_phase(o.decrypt_phase(back, sk)))
    assert np.array_equal(dec.astype(object) % t, want % t)
