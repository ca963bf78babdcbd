"""he355_combine_scalars and he355_ckks_eval_poly on the device, bit for bit against tests/ckks_eval_poly_ref.py (which
tests/test_ckks_eval_poly_ref_cpu.py holds to the oracle's own calls), with sentinels around every output and the operands re-read:

* he355_combine_scalars at N = 1024 (two blocks per row) and 2048 on {60, 40, 40, 60}, {60, 60, 60} and {42, 38, 45, 44}: every level,
  sizes 2 and 3, n = 1, 3 and 5 with he355_set_chunk(2), terms at mixed levels L_t > L, a repeated pointer, a constant (on polynomial 0
  only) and none, edged operands; 257 terms under the 60-bit chain with every operand and scalar q - 1 (one fold of the 128-bit sums); one
  N = 32768, n = 1, L = 2 case for the index width; the same bits as he355_multiply_plain + he355_add + he355_add_plain on the device;
* he355_ckks_eval_poly at degrees 1, 3, 7 (odd only), 8 and 15 for log_baby 1 and 2 on N = 2048 {60, 40 x 5, 60} and N = 4096
  {60, 45 x 5, 60} (both fp64 widths and the u64 prime 0), n = 1 and 5 with he355_set_chunk(2): every ciphertext against the reference,
  he355_poly_stats equal to the plan times its chunks; two calls back to back without a sync; the real-key
  sigmoid decoded within the bound of the CPU test.  The allocator-error path (the block does not fit: the allocator's error before the
  first launch) is argued in DESIGN.md, not provoked here.
These tests fail on a library without the calls: the symbols do not exist."""
import zlib

import numpy as np
import pytest

import ckks_eval_poly_ref as ref
from bfv_gpu_helpers import SENT, At, be, inner_of, sentinelled  # noqa: F401 (be: the fixture)
from test_ckks_eval_poly_ref_cpu import FACTOR, SIGMOID, accuracy

pytestmark = pytest.mark.gpu

COMBINE = {f"n{N}_{'_'.join(map(str, bits))}": (N, bits) for N in (1024, 2048) for bits in ([60, 40, 40, 60], [60, 60, 60], [42, 38, 45, 44])}
EVAL = {"n2048_40": (2048, [60, 40, 40, 40, 40, 40, 60]), "n4096_45": (4096, [60, 45, 45, 45, 45, 45, 60])}
SCALES = {"n2048_40": 2.0 ** 40, "n4096_45": 2.0 ** 45}
POLYS = {
    "deg1": [0.25, -1.5],
    "deg3": SIGMOID,
    "deg7_odd": [0.0, 0.31831, 0.0, -0.10610, 0.0, 0.06366, 0.0, -0.04547],
    "deg8": [0.3 + 0.01 * k for k in range(9)],
    "deg15": [0.2 - 0.01 * k for k in range(16)],
}


def contexts(be, oracle, N, bits):
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    assert g.moduli == o.moduli
    return g, o


@pytest.fixture(scope="module", params=list(COMBINE))
def cctx(request, be, oracle):
    g, o = contexts(be, oracle, *COMBINE[request.param])
    yield g, o, np.random.default_rng(zlib.crc32(request.param.encode()))
    g.close()


def rand_cts(o, rng, n, L, size):
    c = np.stack([o.random_poly(rng, L, size) for _ in range(n)])
    for i, q in enumerate(o.moduli[:L]):  # edged rows: all q - 1, all zero
        c[n - 1, size - 1, i, :] = q - 1
        c[0, 0, i, ::2] = 0
    return c


def run_combine(g, L, size, terms, scalars, const):
    """terms: host arrays [n][size][L_t][N] (an int names an earlier term: the same device slab).  -> [n][size][L][N]"""
    N = g.N
    bufs, dev = [], []
    for t in terms:
        if isinstance(t, int):
            dev.append(dev[t])
        else:
            bufs.append(g.to_device(t))
            dev.append((bufs[-1], t.shape[2]))
    n = next(t for t in terms if not isinstance(t, int)).shape[0]
    d_out = sentinelled(g, n * size * L * N, N)
    g.combine_scalars(L, size, n, dev, scalars, At(d_out, N), const)
    got = inner_of(d_out, N, "d_out").reshape(n, size, L, N)
    host = [t for t in terms if not isinstance(t, int)]
    for b, t in zip(bufs, host):
        assert np.array_equal(b.download(t.shape), t), "a term changed"
        b.free()
    d_out.free()
    return got


def host_terms(terms):
    return [terms[t] if isinstance(t, int) else t for t in terms]


def test_combine_on_every_level_and_size(cctx):
    g, o, rng = cctx
    q = o.moduli
    g.set_chunk(2)
    try:
        for L in range(1, g.L + 1):
            for size, n in ((2, 1), (3, 3), (2, 5)):
                levels = [L, g.L, min(L + 1, g.L)]
                terms = [rand_cts(o, rng, n, lv, size) for lv in levels] + [0]  # the last term repeats the first slab
                scalars = [[int(rng.integers(0, q[i])) for i in range(L)], [q[i] - 1 for i in range(L)], [1] * L, [int(rng.integers(0, q[i])) for i in range(L)]]
                for const in (None, [q[i] - 1 for i in range(L)]):
                    got = run_combine(g, L, size, terms, scalars, const)
                    ht = host_terms(terms)
                    for c in range(n):
                        want = ref.combine(q, L, [t[c] for t in ht], scalars, const)
                        assert np.array_equal(got[c], want), (L, size, n, const is not None, "ciphertext", c)
                    if const is not None:  # the constant lands on polynomial 0 alone
                        bare = run_combine(g, L, size, terms, scalars, None)
                        assert np.array_equal(bare[:, 1:], got[:, 1:]) and not np.array_equal(bare[:, 0], got[:, 0])
    finally:
        g.set_chunk(1024)


def test_combine_one_term_is_a_drop(cctx):
    g, o, rng = cctx
    x = rand_cts(o, rng, 2, g.L, 2)
    got = run_combine(g, 1, 2, [x], [[1]], None)
    assert np.array_equal(got, x[:, :, :1])


def test_combine_257_terms_at_the_edge(cctx):
    g, o, rng = cctx
    q = o.moduli
    L, N = g.L, g.N
    full = np.stack([np.stack([np.stack([np.full(N, q[i] - 1, dtype=np.uint64) for i in range(L)])] * 2)])
    for terms in (256, 257):
        got = run_combine(g, L, 2, [full] + [0] * (terms - 1), [[q[i] - 1 for i in range(L)]] * terms, [q[i] - 1 for i in range(L)])
        for i in range(L):
            assert (got[0, 0, i] == np.uint64((terms * (q[i] - 1) ** 2 + q[i] - 1) % q[i])).all(), (terms, i)
            assert (got[0, 1, i] == np.uint64((terms * (q[i] - 1) ** 2) % q[i])).all(), (terms, i)


def test_combine_equals_multiply_plain_and_add_on_the_device(cctx):
    g, o, rng = cctx
    q = o.moduli
    L, N, n = g.L, g.N, 3
    a, b = rand_cts(o, rng, n, L, 2), rand_cts(o, rng, n, L, 2)
    sa, sb, cst = [int(rng.integers(0, q[i])) for i in range(L)], [q[i] - 1 for i in range(L)], [int(rng.integers(0, q[i])) for i in range(L)]
    got = run_combine(g, L, 2, [a, b], [sa, sb], cst)
    flat = lambda s: np.repeat(np.array(s, dtype=np.uint64)[:, None], N, axis=1)
    da, db, pa, pb, pc = g.to_device(a), g.to_device(b), g.to_device(flat(sa)), g.to_device(flat(sb)), g.to_device(flat(cst))
    ta, tb = g.alloc(a.size), g.alloc(a.size)
    one = g.outer(0, n, 0, 1)  # ciphertext r, the one plaintext
    g.multiply_plain(L, 2, n, da, pa, one, ta)
    g.multiply_plain(L, 2, n, db, pb, one, tb)
    g.add(L, 2, n, ta, tb, g.pairwise(), ta)
    g.add_plain(L, 2, n, ta, pc, one, ta)
    assert np.array_equal(ta.download(a.shape), got)
    for x in (da, db, pa, pb, pc, ta, tb):
        x.free()


def test_combine_at_n32768(be, oracle):
    g, o = contexts(be, oracle, 32768, [60, 40, 40, 60])
    rng = np.random.default_rng(32768)
    q = o.moduli
    L = 2
    terms = [rand_cts(o, rng, 1, 3, 2), rand_cts(o, rng, 1, 2, 2)]
    scalars, const = [[q[0] - 1, 12345], [int(rng.integers(0, q[0])), q[1] - 1]], [7, q[1] - 1]
    got = run_combine(g, L, 2, terms, scalars, const)
    assert np.array_equal(got[0], ref.combine_composed(o, L, [t[0] for t in terms], scalars, const))
    g.close()


# ---- he355_ckks_eval_poly -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(EVAL))
def ectx(request, be, oracle):
    g, o = contexts(be, oracle, *EVAL[request.param])
    rng = np.random.default_rng(zlib.crc32(request.param.encode()))
    rk = o.random_kswitch_key(rng)
    g.set_relin_key(rk)
    yield g, o, rng, rk, SCALES[request.param]
    g.close()


def run_eval(g, L, cts, coeffs, log_baby, s_in, s_out, L_out):
    n, N = len(cts), g.N
    d_in = g.to_device(cts)
    d_out = sentinelled(g, n * 2 * L_out * N, N)
    g.ckks_eval_poly(L, n, d_in, coeffs, log_baby, s_in, s_out, At(d_out, N))
    got = inner_of(d_out, N, "d_out").reshape(n, 2, L_out, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    d_in.free()
    d_out.free()
    return got


@pytest.mark.parametrize("log_baby", [1, 2])
@pytest.mark.parametrize("poly", list(POLYS))
def test_eval_poly_against_the_reference(ectx, poly, log_baby):
    g, o, rng, rk, scale = ectx
    coeffs, L = POLYS[poly], g.L
    g.set_chunk(2)
    try:
        for n in (1, 5):
            cts = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
            pl = g.ckks_eval_poly_plan(L, coeffs, log_baby, scale, scale, n)
            assert pl["chunks"] == (n + 1) // 2
            g.poly_stats(reset=True)
            got = run_eval(g, L, cts, coeffs, log_baby, scale, scale, pl["L_out"])
            st = g.poly_stats()
            assert st["calls"] == 1 and st["chunks"] == pl["chunks"]
            for k in ("products", "combinations", "rescales", "drops", "adds"):
                assert st[k] == pl[k] * pl["chunks"], (k, st, pl)
            for c in range(n):
                want, ev = ref.eval_poly(o, cts[c], coeffs, log_baby, scale, scale, rk, composed=True)
                assert ev.counters() == {k: pl[k] for k in ev.counters()}
                assert np.array_equal(got[c], want), (poly, log_baby, n, "ciphertext", c)
    finally:
        g.set_chunk(1024)


def test_eval_poly_twice_without_a_sync(ectx):
    g, o, rng, rk, scale = ectx
    L, N = g.L, g.N
    a, b = np.stack([o.random_poly(rng, L, 2) for _ in range(2)]), np.stack([o.random_poly(rng, L, 2)])
    pa, pb = POLYS["deg7_odd"], POLYS["deg3"]
    la, lb = g.ckks_eval_poly_plan(L, pa, 1, scale, scale, 2)["L_out"], g.ckks_eval_poly_plan(L, pb, 2, scale, scale, 1)["L_out"]
    da, db = g.to_device(a), g.to_device(b)
    oa, ob = sentinelled(g, 2 * 2 * la * N, N), sentinelled(g, 2 * lb * N, N)
    g.ckks_eval_poly(L, 2, da, pa, 1, scale, scale, At(oa, N))
    g.ckks_eval_poly(L, 1, db, pb, 2, scale, scale, At(ob, N))
    ga, gb = inner_of(oa, N, "first").reshape(2, 2, la, N), inner_of(ob, N, "second").reshape(1, 2, lb, N)
    for c in range(2):
        assert np.array_equal(ga[c], ref.eval_poly(o, a[c], pa, 1, scale, scale, rk, composed=True)[0]), ("first", c)
    assert np.array_equal(gb[0], ref.eval_poly(o, b[0], pb, 2, scale, scale, rk, composed=True)[0]), "second"
    for x in (da, db, oa, ob):
        x.free()


def test_the_relinearization_key_is_asked_for_before_anything_is_allocated(be, oracle):
    g, o = contexts(be, oracle, *EVAL["n2048_40"])
    rng = np.random.default_rng(3)
    x = g.to_device(np.stack([o.random_poly(rng, g.L, 2)]))
    out = g.alloc(2 * g.L * g.N)
    before = g.alloc_stats()
    with pytest.raises(be.HE355Error) as ei:
        g.ckks_eval_poly(g.L, 1, x, SIGMOID, 1, 2.0 ** 40, 2.0 ** 40, out)
    assert "relinearization key not present" in str(ei.value)
    assert g.alloc_stats() == before and g.poly_stats()["calls"] == 0
    g.close()


def test_the_real_key_sigmoid_decodes_within_the_bound(be, oracle):
    import oracle as ho
    N, bits, scale, seed = 2048, [60, 40, 40, 40, 40, 60], 2.0 ** 40, 100
    tree_cpu, hor = accuracy(bits, SIGMOID, seed)  # the CPU test's case: the same seeds, the same ciphertext
    g, o = contexts(be, oracle, N, bits)
    vals = np.random.default_rng(seed).uniform(-1.0, 1.0, N // 2)
    sk = o.keygen_secret(seed)
    pk, rk = o.keygen_public(sk, seed + 1), o.keygen_relin(sk, seed + 2)
    x = o.encrypt(pk, ho.ckks_encode(o, vals, scale), seed + 3)
    g.set_relin_key(rk)
    pl = g.ckks_eval_poly_plan(g.L, SIGMOID, 1, scale, scale, 1)
    got = run_eval(g, g.L, x[None], SIGMOID, 1, scale, scale, pl["L_out"])[0]
    err = float(np.max(np.abs(ho.ckks_decode(o, o.decrypt_phase(got, sk), scale).real - np.polyval(SIGMOID[::-1], vals))))
    print(f"sigmoid on the device: {err:.3e}  (reference tree {tree_cpu:.3e}, horner {hor:.3e})")
    assert err == tree_cpu  # the same bits as the reference decode to the same slots
    assert err <= FACTOR * hor
    g.close()
