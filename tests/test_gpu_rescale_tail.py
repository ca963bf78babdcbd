"""multiply -> relinearize -> rescale on the fused throughput shape, both orders of its rescale tail, bit for bit against the oracle.

With `out` apart from the operands k_k3 forms c0, c1 from the operand rows and the divided-out prime takes the short order (its tiles
leave through the inverse row pass, k_floor_colsn subtracts P^-1 * delta1 in coefficient form: K3Fuse::raw_tail, launch_floor_cols'
sub2); with `out` overlapping an operand k_k1 writes c0, c1 and the tail keeps the present order (correction column pass, floor step in
NTT form, k_rows_inv_select).  Both must give the oracle's ciphertexts -- at small rings whose divided-out prime sits on the fp64
engine, on the u64 engine's fold form and on its Shoup form, and at the bench ring N = 2^15, L = 16.
The exact-integer statement of the identity: tests/test_rescale_tail_identity.py."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import shoup_rings as shoup  # noqa: E402

pytestmark = pytest.mark.gpu

# (as tests/test_gpu_bench_shapes.py: the path counters describe the library's own choice of shape)
_SHAPE_ENV = ("HE355_CHUNK", "HE355_LATENCY_MAX", "HE355_LEVEL_WALK", "HE355_LDS_MAX", "HE355_FORCE_U64")
DEFAULT_SHAPES = not any(os.environ.get(k) for k in _SHAPE_ENV)


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need an MI355X (the backend has no CPU fallback)")
    return mod


# (N, key-level bits, sec128, batch, engine of the divided-out prime, result rows held to the oracle)
CASES = {
    "n4096_last_prime_fp64": (4096, [60, 45, 45, 60], False, 256, True, None),
    "n4096_last_prime_u64_fold": (4096, [60, 45, 60, 60], False, 256, False, None),
    "n4096_last_prime_u64_shoup": (4096, [50, 50, 50, 50], False, 256, False, None),
    "n32768_l16_bench_ring": (32768, [60] + [45] * 15 + [60], True, 32, True, (0, 1, 15, 31)),
    # the Shoup build at LOGN1 = 4 (tests/shoup_rings.py); fused from 57 ciphertexts at N = 16384 (16 x ceil(n / 8) >= 128 blocks)
    "n16384_60_50_40_60_shoup": (16384, [60, 50, 40, 60], False, 64, True, None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_both_orders_of_the_rescale_tail_equal_the_oracle(be, oracle, case):
    N, bits, sec128, n, last_fp64, rows = CASES[case]
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=sec128, device=0)
    try:
        o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=sec128)
        assert g.moduli == o.moduli
        if case in shoup.RINGS:
            shoup.check_device(case, g)
        rng = np.random.default_rng(N + n)
        L = g.L
        assert L == len(bits) - 1
        rk = o.random_kswitch_key(rng)
        g.set_relin_key(rk)
        a = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
        b = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
        rows = range(n) if rows is None else rows
        want = {r: o.rescale(o.relinearize(o.multiply_ntt(a[r], b[r]), rk)) for r in rows}
        da, db = g.to_device(a), g.to_device(b)
        # short order: `out` a slab of its own
        out = g.alloc(n * 2 * (L - 1) * N)
        g.path_stats(reset=True)
        g.multiply_relin(L, n, da, db, be.Context.pairwise(), out, rescale=True)
        g.sync()
        st = g.path_stats()
        got = out.download((n, 2, L - 1, N))
        for r in rows:
            assert np.array_equal(got[r], want[r]), ("out apart", r)
        if DEFAULT_SHAPES:
            assert bool(g.fp64[L - 1]) == last_fp64
            assert st["ks_fused"] >= 1 and all(st[k] == 0 for k in ("ks_unfused", "ks_latency", "ks_lds")), st
        # the operands were only read
        assert np.array_equal(da.download((n, 2, L, N)), a) and np.array_equal(db.download((n, 2, L, N)), b)
        # present order: the result over operand a
        g.path_stats(reset=True)
        g.multiply_relin(L, n, da, db, be.Context.pairwise(), da, rescale=True)
        g.sync()
        st = g.path_stats()
        got2 = da.download_head((n, 2, L - 1, N))
        for r in rows:
            assert np.array_equal(got2[r], want[r]), ("out over operand a", r)
        assert np.array_equal(got2, got), "the two orders of the rescale tail disagree"
        if DEFAULT_SHAPES:
            assert st["ks_fused"] >= 1 and all(st[k] == 0 for k in ("ks_unfused", "ks_latency", "ks_lds")), st
    finally:
        g.close()
