"""The definition of the BFV ciphertext merge (he355_bfv_merge; tests/bfv_merge_ref.py::merge_levels, the reference of the GPU tests) run in
the oracle, and what it decrypts to:

* fresh oracle.encrypt inputs with full-range plaintexts merge into a ciphertext whose coefficient k + 2^d m is 2^d mu_(k, 2^d m) mod t for
  k < count and 0 for count <= k < 2^d, with no wrong coefficient: (1024, {50, 40, 50}, t of 20 bits) at count 5, 8 and 16,
  (2048, {60, 40, 60}) at count 2048, all 11 levels, and (1024, {45, 55, 50}) at count 5;
* merge(expand(q)) at count 8 on n1024 decrypts to 64 m.
No GPU."""
import numpy as np
import pytest

from bfv_expand_ref import children, expand_levels
from bfv_merge_ref import decrypt, merge_levels, merged_plain

SHAPES = [((1024, [50, 40, 50], 20), 5), ((1024, [50, 40, 50], 20), 8), ((1024, [50, 40, 50], 20), 16), ((2048, [60, 40, 60], 20), 2048),
          ((1024, [45, 55, 50], 20), 5)]  # the last: an fp64 prime 0 beside a u64 one (test_gpu_bfv_chain_layouts.py)


def keyed(oracle, chain, count, seed):
    N, bits, pb = chain
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    sk = o.keygen_secret(21)
    pk = o.keygen_public(sk, 22)
    gks = {}
    for j in range((count - 1).bit_length()):
        e = N // (1 << j) + 1
        gks[e] = o.keygen_galois(sk, e, seed + j)
    return o, sk, pk, gks


def shape_id(chain, count):
    """n<N>-count<k>; a chain other than the two first ones also names its bit sizes, so that no two shapes share an id"""
    tag = "" if chain[1] in ([50, 40, 50], [60, 40, 60]) else "-" + "_".join(str(b) for b in chain[1])
    return f"n{chain[0]}{tag}-count{count}"


@pytest.mark.parametrize("chain,count", SHAPES, ids=[shape_id(c, k) for c, k in SHAPES])
def test_merge_decrypts_to_the_closed_form(oracle, chain, count):
    o, sk, pk, gks = keyed(oracle, chain, count, 300)
    N, t, L = o.N, o.t, o.L
    rng = np.random.default_rng(70 + count)
    mu = rng.integers(0, t, (count, N), dtype=np.uint64)
    mu[0, :4] = [0, 1, t - 1, t // 2]
    cts = [o.encrypt(pk, mu[k], 400 + k) for k in range(count)]
    got = decrypt(o, sk, merge_levels(o, cts, count, gks, L))
    want = merged_plain(mu, t)
    d = (count - 1).bit_length()
    for k in range(count, 1 << d):
        assert not want[k::1 << d].any()
    assert np.array_equal(got, want), int((got != want).sum())


def test_merge_of_expand_is_four_to_the_d(oracle):
    count = 8
    o, sk, pk, gks = keyed(oracle, (1024, [50, 40, 50], 20), count, 320)
    N, t, L = o.N, o.t, o.L
    m = np.random.default_rng(71).integers(0, t, N, dtype=np.uint64)
    kids = children(expand_levels(o, o.encrypt(pk, m, 401), 3, gks, L), count)
    got = decrypt(o, sk, merge_levels(o, kids, count, gks, L))
    assert np.array_equal(got, (m.astype(object) * 64 % t).astype(np.uint64))
