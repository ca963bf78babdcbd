"""The pool blocks the BFV calls hold for the length of a call (device_pool.h, PoolBlock) go back to the pool when the call returns: for each
of the nine holders, at the smallest shape that takes its block, he355_alloc_stats around the call shows

* the call took at least the blocks it is known to hold (pool hits + misses went up by that many);
* live_bytes is back at its value from before the call;
* a second identical call makes no raw allocation (the blocks come off the free lists) and again leaves live_bytes where it was.

  he355_bfv_multiply_relin_accumulate              2 x 2 x 2 at N = 2048: the products and the relinearized terms, two blocks
  he355_bfv_expand                                 N = 2048, count 4 (two levels), n = 2: the level in between
  he355_bfv_decompose_ntt, _unpack_bytes_ntt       N = 1024, the routed path (asserted by he355_bfv_route_stats), n = 2: the coefficient slab
  he355_bfv_rgsw_encrypt, _selector_encrypt        N = 2048, one level below the top: the encryptions of zero
  he355_bfv_rgsw_encrypt_secret                    N = 2048 at the top level (the secret's coefficients) and one below (the inner call's zeros too)
  he355_bfv_external_product                       N = 2048, n = 2, inner = 2: the digit slab
  he355_bfv_rgsw_from_bfv                          N = 2048, n = 1, n_sel = 1: the digit slab

What the calls compute is held to the oracle by test_gpu_bfv_{multiply_routes,expand,digits,bytes,external_product,selectors}.py; the
operands here are small canonical values and the results are not read."""
import numpy as np
import pytest

from bfv_gpu_helpers import be, pair  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
V = 20


def held(g, call, blocks):
    """run `call` twice; `blocks`: the pool blocks one call is known to take"""
    g.sync()
    s0 = g.alloc_stats()
    call()
    s1 = g.alloc_stats()
    assert s1["pool_hits"] + s1["pool_misses"] - s0["pool_hits"] - s0["pool_misses"] >= blocks, (s0, s1)
    assert s1["live_bytes"] == s0["live_bytes"], (s0, s1)
    call()
    s2 = g.alloc_stats()
    assert s2["raw_mallocs"] == s1["raw_mallocs"], (s1, s2)
    assert s2["pool_hits"] - s1["pool_hits"] >= blocks and s2["pool_misses"] == s1["pool_misses"], (s1, s2)
    assert s2["live_bytes"] == s0["live_bytes"], (s0, s2)
    g.sync()


def small(g, rng, words, bound=1 << 30):
    """canonical residues under every prime of the chains here (all above 2^30)"""
    return g.to_device(rng.integers(0, bound, words, dtype=np.uint64))


@pytest.fixture(scope="module")
def g2048(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, N2048, keys=True)
    g.set_relin_key_synthetic(7)
    for j, e in enumerate(g.bfv_expand_galois_elts(4)):
        g.set_galois_key_synthetic(e, 8 + j)
    yield g
    g.close()


@pytest.fixture(scope="module")
def g1024(be, oracle):
    g = pair(be, oracle, "n1024")[0]
    yield g
    g.close()


def test_multiply_relin_accumulate(g2048):
    g, N, L = g2048, g2048.N, g2048.L
    rng = np.random.default_rng(1)
    a, b, out = small(g, rng, 4 * 2 * L * N), small(g, rng, 4 * 2 * L * N), g.alloc(4 * 2 * L * N)
    held(g, lambda: g.bfv_multiply_relin_accumulate(L, 2, 2, 2, a, 1, 2, b, 2, 1, out), 2)


def test_expand(g2048):
    g, N, L = g2048, g2048.N, g2048.L
    inp, out = small(g, np.random.default_rng(2), 2 * 2 * L * N), g.alloc(4 * 2 * 2 * L * N)
    held(g, lambda: g.bfv_expand(L, 2, inp, 4, out), 1)


def test_decompose_ntt_routed(g1024):
    g, N, L = g1024, g1024.N, g1024.L
    F = 2 * g.bfv_digit_count(L)[0]
    ct, out = small(g, np.random.default_rng(3), 2 * 2 * L * N), g.alloc(2 * F * L * N)
    g.bfv_route_stats(reset=True)
    held(g, lambda: g.bfv_decompose_ntt(L, 2, 2, ct, L, out), 1)
    r = g.bfv_route_stats()
    assert r["digits_routed"] == 2 and r["digits_fused"] == 0, r


def test_unpack_bytes_ntt_routed(g1024):
    g, N, L = g1024, g1024.N, g1024.L
    B = g.bfv_bytes_per_plain()[0]
    buf, out = small(g, np.random.default_rng(4), (2 * B + 7) // 8, 1 << 63), g.alloc(2 * L * N)
    g.bfv_route_stats(reset=True)
    held(g, lambda: g.bfv_unpack_bytes_ntt(L, 2, buf, 0, B, B, out), 1)
    r = g.bfv_route_stats()
    assert r["bytes_routed"] == 2 and r["bytes_fused"] == 0, r


def test_rgsw_encrypt_below_the_top(g2048):
    g, N, L = g2048, g2048.N, g2048.L - 1
    E = g.bfv_gadget_count(L, V)[0]
    plain, out = small(g, np.random.default_rng(5), N, 1000), g.alloc(2 * E * 2 * L * N)
    held(g, lambda: g.bfv_rgsw_encrypt(L, V, 1, plain, 31, 0, out), 1)


def test_selector_encrypt_below_the_top(g2048):
    g, N, L = g2048, g2048.N, g2048.L - 1
    E = g.bfv_gadget_count(L, V)[0]
    sel, out = small(g, np.random.default_rng(6), 1, 2), g.alloc(2 * L * N)
    held(g, lambda: g.bfv_selector_encrypt(L, V, 1, 1, 0, E, sel, 32, 0, out), 1)


@pytest.mark.parametrize("below", [0, 1], ids=["top", "below"])
def test_rgsw_encrypt_secret(g2048, below):
    g, N, L = g2048, g2048.N, g2048.L - below
    E = g.bfv_gadget_count(L, V)[0]
    out = g.alloc(2 * E * 2 * L * N)
    held(g, lambda: g.bfv_rgsw_encrypt_secret(L, V, 33, 0, out), 1 + below)


def test_external_product(g2048):
    g, N, L = g2048, g2048.N, g2048.L
    E = g.bfv_gadget_count(L, V)[0]
    rng = np.random.default_rng(7)
    ct, rgsw, out = small(g, rng, 4 * 2 * L * N), small(g, rng, 4 * 2 * E * 2 * L * N), g.alloc(2 * 2 * L * N)
    held(g, lambda: g.bfv_external_product(L, V, 2, 2, ct, 2, 1, rgsw, 2, 1, out), 1)


def test_rgsw_from_bfv(g2048):
    g, N, L = g2048, g2048.N, g2048.L
    E = g.bfv_gadget_count(L, V)[0]
    rng = np.random.default_rng(8)
    ct, key, out = small(g, rng, E * 2 * L * N), small(g, rng, 2 * E * 2 * L * N), g.alloc(2 * E * 2 * L * N)
    held(g, lambda: g.bfv_rgsw_from_bfv(L, V, V, 1, 1, ct, 1, 1, key, out), 1)
