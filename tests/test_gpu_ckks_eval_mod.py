"""he355_combine_scalars_rescale, he355_ckks_eval_chebyshev and he355_ckks_eval_mod on the device, bit for bit against
tests/ckks_eval_mod_ref.py (which tests/test_ckks_eval_mod_ref_cpu.py holds to the oracle's own calls), with sentinels around every output
and the operands re-read:

* the fused step at N = 1024 and 2048 on {60, 40, 40, 60}, {60, 60, 60}, {42, 38, 45, 44} and the Shoup-form chain shoup_by_one_low60 of
  tests/golden/explicit_moduli.json: every L from 2 to L_top, sizes 2 and 3, n = 1, 3 and 5 under he355_set_chunk(2), terms at mixed levels
  and a repeated pointer, with and without a constant, under he355_set_latency_max(0) and the default; 257 terms of q - 1 times q - 1 on
  the 60-bit chain; a one-term, scalar-1 case whose last row holds the coefficients 0, floor(q/2), floor(q/2) + 1 and q - 1 -- the edges of
  the rescale's floor -- from tests/edge_operands.py; one N = 32768, L = 2, n = 1 case.  Every result equals the reference AND the device's
  own he355_combine_scalars + he355_rescale;
* he355_ckks_eval_chebyshev at degrees 1, 2, 3, 7 (odd only), 8 and 15 for log_baby 1, 2 and 3 on N = 2048 {60, 40 x 5, 60} and N = 4096
  {60, 45 x 5, 60}, n = 1 and 5 with he355_set_chunk(2): every ciphertext against the reference, he355_cheb_stats equal to the plan times
  its chunks, he355_poly_stats unmoved; two calls back to back without a sync;
* he355_ckks_eval_mod at (K = 3, r = 2, degree 15) on N = 2048 {60, 40 x 7, 60}: bit for bit on uniform residues, and with real keys the
  decode within the CPU test's bound (2 x the monomial yardstick's error).
These tests fail on a library without the calls: the symbols do not exist."""
import zlib

import numpy as np
import pytest

import ckks_eval_mod_ref as mref
import edge_operands
import explicit_moduli
from bfv_gpu_helpers import At, be, inner_of, sentinelled  # noqa: F401 (be: the fixture)
from test_ckks_eval_mod_ref_cpu import BITS8, DEGREE, FACTOR, K, R, SCALE, eval_mod_case, slot_error

pytestmark = pytest.mark.gpu

FUSED = {f"n{N}_{'_'.join(map(str, bits))}": (N, bits, None) for N in (1024, 2048) for bits in ([60, 40, 40, 60], [60, 60, 60], [42, 38, 45, 44])}
FUSED["shoup_by_one_low60"] = (2048, None, explicit_moduli.load()["shoup_by_one_low60"]["primes"])
EVAL = {"n2048_40": (2048, [60, 40, 40, 40, 40, 40, 60]), "n4096_45": (4096, [60, 45, 45, 45, 45, 45, 60])}
SCALES = {"n2048_40": 2.0 ** 40, "n4096_45": 2.0 ** 45}
POLYS = {
    "deg1": [0.25, -1.5],
    "deg2": [0.1, 0.0, 0.5],
    "deg3": [0.5, 0.15012, 0.0, -0.0015930078125],
    "deg7_odd": [0.0, 0.31831, 0.0, -0.10610, 0.0, 0.06366, 0.0, -0.04547],
    "deg8": [0.3 + 0.01 * k for k in range(9)],
    "deg15": [0.2 - 0.01 * k for k in range(16)],
}


def contexts(be, oracle, N, bits, primes=None):
    kw = dict(primes=primes) if primes is not None else dict(bit_sizes=bits)
    g = be.Context(be.SCHEME_CKKS, N, sec128=False, device=0, **kw)
    o = oracle.Context(oracle.SCHEME_CKKS, N, sec128=False, **kw)
    assert g.moduli == o.moduli
    return g, o


@pytest.fixture(scope="module", params=list(FUSED))
def fctx(request, be, oracle):
    g, o = contexts(be, oracle, *FUSED[request.param])
    yield g, o, np.random.default_rng(zlib.crc32(request.param.encode()))
    g.close()


def rand_cts(o, rng, n, L, size):
    c = np.stack([o.random_poly(rng, L, size) for _ in range(n)])
    for i, q in enumerate(o.moduli[:L]):  # edged rows: all q - 1, all zero
        c[n - 1, size - 1, i, :] = q - 1
        c[0, 0, i, ::2] = 0
    return c


def run_fused(g, L, size, terms, scalars, const):
    """terms: host arrays [n][size][L_t][N] (an int names an earlier term: the same device slab).  -> [n][size][L - 1][N], which is also
    what the device's own he355_combine_scalars + he355_rescale give"""
    N = g.N
    bufs, dev = [], []
    for t in terms:
        if isinstance(t, int):
            dev.append(dev[t])
        else:
            bufs.append(g.to_device(t))
            dev.append((bufs[-1], t.shape[2]))
    n = next(t for t in terms if not isinstance(t, int)).shape[0]
    d_out = sentinelled(g, n * size * (L - 1) * N, N)
    g.combine_scalars_rescale(L, size, n, dev, scalars, At(d_out, N), const)
    got = inner_of(d_out, N, "d_out").reshape(n, size, L - 1, N)
    tmp, two = g.alloc(n * size * L * N), sentinelled(g, n * size * (L - 1) * N, N)
    g.combine_scalars(L, size, n, dev, scalars, tmp, const)
    g.rescale(L, size, n, tmp, At(two, N))
    assert np.array_equal(inner_of(two, N, "composition").reshape(got.shape), got), "the device's own combine_scalars + rescale"
    host = [t for t in terms if not isinstance(t, int)]
    for b, t in zip(bufs, host):
        assert np.array_equal(b.download(t.shape), t), "a term changed"
        b.free()
    for x in (d_out, tmp, two):
        x.free()
    return got


def host_terms(terms):
    return [terms[t] if isinstance(t, int) else t for t in terms]


def want_fused(o, L, terms, scalars, const, c):
    return mref.combine_rescale(o, L, [t[c] for t in host_terms(terms)], scalars, const, composed=True)


def test_fused_step_on_every_level_and_size(fctx):
    g, o, rng = fctx
    q = o.moduli
    g.set_chunk(2)
    try:
        for L in range(2, g.L + 1):
            for size, n in ((2, 1), (3, 3), (2, 5)):
                levels = [L, g.L, min(L + 1, g.L)]
                terms = [rand_cts(o, rng, n, lv, size) for lv in levels] + [0]  # the last term repeats the first slab
                scalars = [[int(rng.integers(0, q[i])) for i in range(L)], [q[i] - 1 for i in range(L)], [1] * L, [int(rng.integers(0, q[i])) for i in range(L)]]
                for const in (None, [q[i] - 1 for i in range(L)]):
                    g.cheb_stats(reset=True)
                    before = g.poly_stats()
                    got = run_fused(g, L, size, terms, scalars, const)
                    assert g.cheb_stats()["fused_steps"] == 1 and g.cheb_stats()["calls"] == 0
                    assert g.poly_stats()["combinations"] == before["combinations"] + 1  # (the composition's own launch, none of the fused call's)
                    for c in range(n):
                        assert np.array_equal(got[c], want_fused(o, L, terms, scalars, const, c)), (L, size, n, const is not None, "ciphertext", c)
                    g.set_latency_max(0)
                    try:
                        assert np.array_equal(run_fused(g, L, size, terms, scalars, const), got), (L, size, n, "latency shapes off")
                    finally:
                        g.set_latency_max(None)
    finally:
        g.set_chunk(1024)


def test_fused_step_of_one_term_is_the_rescale(fctx):
    g, o, rng = fctx
    L = g.L
    x = rand_cts(o, rng, 2, L, 2)
    got = run_fused(g, L, 2, [x], [[1] * L], None)
    for c in range(2):
        assert np.array_equal(got[c], o.rescale(x[c]))


def test_fused_step_on_the_edges_of_the_floor(fctx):
    g, o, rng = fctx
    L = g.L
    for name in ("zero_coeff", "half_coeff", "half1_coeff", "qm1_coeff"):  # every coefficient of every row: 0, floor(q/2), floor(q/2) + 1, q - 1
        x = np.stack([edge_operands.family(o, name, L, 2), edge_operands.family(o, name, L, 2)])
        x[1, 1] = o.random_poly(rng, L, 1)[0]
        got = run_fused(g, L, 2, [x], [[1] * L], None)
        for c in range(2):
            assert np.array_equal(got[c], o.rescale(x[c])), (name, c)


@pytest.mark.parametrize("N", [1024, 2048])
def test_fused_step_of_257_terms_at_the_edge(be, oracle, N):
    g, o = contexts(be, oracle, N, [60, 60, 60])  # (the 2^128 edge of a run is the 60-bit chain's)
    q = o.moduli
    L = g.L
    full = np.stack([np.stack([np.stack([np.full(N, q[i] - 1, dtype=np.uint64) for i in range(L)])] * 2)])
    for terms in (256, 257):
        cst = [q[i] - 1 for i in range(L)]
        got = run_fused(g, L, 2, [full] + [0] * (terms - 1), [[q[i] - 1 for i in range(L)]] * terms, cst)
        comb = np.empty((2, L, N), dtype=np.uint64)
        for i in range(L):
            comb[0, i] = (terms * (q[i] - 1) ** 2 + q[i] - 1) % q[i]
            comb[1, i] = (terms * (q[i] - 1) ** 2) % q[i]
        assert np.array_equal(got[0], o.rescale(comb)), terms
    g.close()


def test_fused_step_at_n32768(be, oracle):
    g, o = contexts(be, oracle, 32768, [60, 40, 40, 60])
    rng = np.random.default_rng(32768)
    q = o.moduli
    L = 2
    terms = [rand_cts(o, rng, 1, 3, 2), rand_cts(o, rng, 1, 2, 2)]
    scalars, const = [[q[0] - 1, 12345], [int(rng.integers(0, q[0])), q[1] - 1]], [7, q[1] - 1]
    got = run_fused(g, L, 2, terms, scalars, const)
    assert np.array_equal(got[0], want_fused(o, L, terms, scalars, const, 0))
    g.close()


# ---- he355_ckks_eval_chebyshev ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(EVAL))
def ectx(request, be, oracle):
    g, o = contexts(be, oracle, *EVAL[request.param])
    rng = np.random.default_rng(zlib.crc32(request.param.encode()))
    rk = o.random_kswitch_key(rng)
    g.set_relin_key(rk)
    yield g, o, rng, rk, SCALES[request.param]
    g.close()


def run_eval(g, L, cts, coeffs, log_baby, s_in, s_out, L_out, r=None):
    n, N = len(cts), g.N
    d_in = g.to_device(cts)
    d_out = sentinelled(g, n * 2 * L_out * N, N)
    if r is None:
        g.ckks_eval_chebyshev(L, n, d_in, coeffs, log_baby, s_in, s_out, At(d_out, N))
    else:
        g.ckks_eval_mod(L, n, d_in, coeffs, log_baby, s_in, s_out, r, At(d_out, N))
    got = inner_of(d_out, N, "d_out").reshape(n, 2, L_out, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    d_in.free()
    d_out.free()
    return got


STAT_KEYS = {"products": "products", "fused_steps": "rescales", "combinations": "combinations", "drops": "drops", "adds": "adds", "double_angles": "double_angles"}


def check_stats(g, pl):
    st = g.cheb_stats()
    assert st["calls"] == 1 and st["chunks"] == pl["chunks"]
    for k, p in STAT_KEYS.items():
        assert st[k] == pl[p] * pl["chunks"], (k, st, pl)


@pytest.mark.parametrize("log_baby", [1, 2, 3])
@pytest.mark.parametrize("poly", list(POLYS))
def test_eval_chebyshev_against_the_reference(ectx, poly, log_baby):
    g, o, rng, rk, scale = ectx
    coeffs, L = POLYS[poly], g.L
    cts = np.stack([o.random_poly(rng, L, 2) for _ in range(5)])
    want = []
    for c in range(5):
        w, ev = mref.eval_chebyshev(o, cts[c], coeffs, log_baby, scale, scale, rk, composed=True)
        want.append(w)
    g.set_chunk(2)
    try:
        for n in (1, 5):
            pl = g.ckks_eval_chebyshev_plan(L, coeffs, log_baby, scale, scale, n)
            assert pl["chunks"] == (n + 1) // 2 and ev.counters() == {k: pl[k] for k in ev.counters()}
            g.cheb_stats(reset=True)
            poly_before = g.poly_stats()
            got = run_eval(g, L, cts[:n], coeffs, log_baby, scale, scale, pl["L_out"])
            check_stats(g, pl)
            assert g.poly_stats() == poly_before
            for c in range(n):
                assert np.array_equal(got[c], want[c]), (poly, log_baby, n, "ciphertext", c)
    finally:
        g.set_chunk(1024)


def test_eval_chebyshev_twice_without_a_sync(ectx):
    g, o, rng, rk, scale = ectx
    L, N = g.L, g.N
    a, b = np.stack([o.random_poly(rng, L, 2) for _ in range(2)]), np.stack([o.random_poly(rng, L, 2)])
    pa, pb = POLYS["deg7_odd"], POLYS["deg3"]
    la, lb = g.ckks_eval_chebyshev_plan(L, pa, 1, scale, scale, 2)["L_out"], g.ckks_eval_chebyshev_plan(L, pb, 2, scale, scale, 1)["L_out"]
    da, db = g.to_device(a), g.to_device(b)
    oa, ob = sentinelled(g, 2 * 2 * la * N, N), sentinelled(g, 2 * lb * N, N)
    g.ckks_eval_chebyshev(L, 2, da, pa, 1, scale, scale, At(oa, N))
    g.ckks_eval_chebyshev(L, 1, db, pb, 2, scale, scale, At(ob, N))
    ga, gb = inner_of(oa, N, "first").reshape(2, 2, la, N), inner_of(ob, N, "second").reshape(1, 2, lb, N)
    for c in range(2):
        assert np.array_equal(ga[c], mref.eval_chebyshev(o, a[c], pa, 1, scale, scale, rk, composed=True)[0]), ("first", c)
    assert np.array_equal(gb[0], mref.eval_chebyshev(o, b[0], pb, 2, scale, scale, rk, composed=True)[0]), "second"
    for x in (da, db, oa, ob):
        x.free()


def test_the_relinearization_key_is_asked_for_before_anything_is_allocated(be, oracle):
    g, o = contexts(be, oracle, *EVAL["n2048_40"])
    rng = np.random.default_rng(3)
    x = g.to_device(np.stack([o.random_poly(rng, g.L, 2)]))
    out = g.alloc(2 * g.L * g.N)
    before = g.alloc_stats()
    with pytest.raises(be.HE355Error) as ei:
        g.ckks_eval_mod(g.L, 1, x, POLYS["deg3"], 1, 2.0 ** 40, 2.0 ** 40, 1, out)
    assert "relinearization key not present" in str(ei.value)
    assert g.alloc_stats() == before and g.cheb_stats()["calls"] == 0
    g.close()


# ---- he355_ckks_eval_mod ------------------------------------------------------------------------------------------------------------------
def test_eval_mod_against_the_reference(be, oracle):
    g, o = contexts(be, oracle, 2048, BITS8)
    rng = np.random.default_rng(77)
    rk = o.random_kswitch_key(rng)
    g.set_relin_key(rk)
    L, coeffs = g.L, be.eval_mod_coeffs(K, R, DEGREE)
    assert coeffs == mref.eval_mod_coeffs(K, R, DEGREE)
    cts = np.stack([o.random_poly(rng, L, 2) for _ in range(3)])
    g.set_chunk(2)
    pl = g.ckks_eval_mod_plan(L, coeffs, 1, SCALE, SCALE, R, 3)
    assert (pl["depth"], pl["L_out"], pl["double_angles"], pl["chunks"]) == (4 + R, L - 4 - R, R, 2)
    got = run_eval(g, L, cts, coeffs, 1, SCALE, SCALE, pl["L_out"], r=R)
    check_stats(g, pl)
    for c in range(3):
        want, mv = mref.eval_mod(o, cts[c], coeffs, 1, SCALE, SCALE, R, rk, composed=True)
        assert mv.counters() == {k: pl[k] for k in mv.counters()} and mv.out_scale == pl["out_scale"]
        assert np.array_equal(got[c], want), ("ciphertext", c)
    # r = 0 is the Chebyshev call
    g.set_chunk(1024)
    l0 = g.ckks_eval_chebyshev_plan(L, coeffs, 1, SCALE, SCALE, 1)["L_out"]
    assert np.array_equal(run_eval(g, L, cts[:1], coeffs, 1, SCALE, SCALE, l0, r=0), run_eval(g, L, cts[:1], coeffs, 1, SCALE, SCALE, l0))
    g.close()


def test_the_real_key_eval_mod_decodes_within_the_bound(be, oracle):
    g, o = contexts(be, oracle, 2048, BITS8)
    sk = o.keygen_secret(300)  # the CPU test's keys and case: the same seeds, the same ciphertext
    pk, rk = o.keygen_public(sk, 301), o.keygen_relin(sk, 302)
    u, v, c, x, want = eval_mod_case(o, pk, 400)
    g.set_relin_key(rk)
    pl = g.ckks_eval_mod_plan(g.L, c, 1, SCALE, SCALE, R, 1)
    got = run_eval(g, g.L, x[None], c, 1, SCALE, SCALE, pl["L_out"], r=R)[0]
    yard, ys = mref.yardstick(o, x, c, 1, SCALE, SCALE, R, rk)
    err, e_yard = slot_error(o, sk, got, pl["out_scale"], want), slot_error(o, sk, yard, ys, want)
    e_sin = slot_error(o, sk, got, pl["out_scale"], np.sin(2.0 * np.pi * v))
    print(f"eval mod on the device: {err:.3e}  (monomial yardstick {e_yard:.3e}, against sin(2 pi v) {e_sin:.3e})")
    assert err <= FACTOR * e_yard
    assert e_sin < 1e-3
    g.close()
