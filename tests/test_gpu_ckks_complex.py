"""Complex CKKS slots on the device (run with -m gpu on an MI355X), bit for bit against tests/ckks_complex_ref.py and the host client, with
sentinels around every output and the operands re-read:

* the codec at N = 1024 and 4096, n = 3, count = 1, N/2 - 1 and N/2: he355_ckks_encode_complex equals the host client, and with im = 0
  he355_ckks_encode; the fixture's row within the real encoder's bound of the exact coefficients; the re parts of
  he355_ckks_decode_complex equal he355_ckks_decode, the pairs equal the host client's; the round trip inside N / scale; one _slots call with
  two ranges; the decode cases of tests/golden/ckks_complex_vectors.json within the real decoder's bound, part by part;
* he355_combine_scalars_complex at N = 1024 (the sign changes between the waves of one block), 2048 (a block is exactly one quarter) and
  4096 on {60, 40, 40, 60}, and on the Shoup-form chain shoup_by_one_low60 of tests/golden/explicit_moduli.json: sizes 2 and 3, n = 1 and 3,
  1, 2 and 257 terms with one term at a higher level and a repeated pointer, with and without a constant, against the Python-integer
  definition; two terms against he355_multiply_plain by NTT(A + B J) plus he355_add on the device; equal halves against
  he355_combine_scalars; he355_poly_stats;
* he355_ckks_eval_poly_complex at N = 2048 for a degree-3 and a degree-7 complex polynomial with log_baby 1 and 2, three ciphertexts in two
  chunks, against the reference, the counters against the plan; zero imaginary parts against he355_ckks_eval_poly;
* two compositions with real keys at N = 1024, each decoded and held to numpy within the noise of its own reference run on the oracle: the
  real and imaginary parts of an encrypted complex vector (he355_apply_galois under 2N - 1, one complex combination per part with the
  scalars W/2 and -+i W/2 on {x, conj x}, he355_rescale), and a complex banded matrix (diagonals through he355_ckks_encode_complex,
  he355_plain_extend_special -- mismatch count 0 -- and he355_linear_transform_bsgs at 2 x 2).
These tests fail on a library without the calls: the symbols do not exist."""
import json
import os
import zlib

import numpy as np
import pytest

import ckks_complex_operands as cx
import ckks_complex_ref as cref
import client_operands as co
import linear_transform_bsgs_ref as bsgs
import rotate_hoisted_lazy_ref as lazy
from bfv_gpu_helpers import SENT, At, be, inner_of, sentinelled  # noqa: F401 (be: the fixture)
from test_ckks_complex_ref_cpu import CUBIC, SEPTIC
from test_linear_transform_bsgs_ref_cpu import CKKS_RATIO_CAP
from test_rotate_hoisted_lazy_ref_cpu import _diagonals

pytestmark = pytest.mark.gpu

BITS = [60, 40, 40, 60]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explicit_moduli.json")) as _f:
    SHOUP = next(c for c in json.load(_f)["chains"] if c["id"] == "shoup_by_one_low60")
COMBINE = {"n1024": (1024, {"bit_sizes": BITS, "sec128": False}), "n2048": (2048, {"bit_sizes": BITS, "sec128": False}),
           "n4096": (4096, {"bit_sizes": BITS, "sec128": False}), "n2048_shoup": (SHOUP["N"], {"primes": [int(p, 16) for p in SHOUP["primes"]]})}


def contexts(be, oracle, N, how):
    g = be.Context(be.SCHEME_CKKS, N, device=0, **how)
    o = oracle.Context(oracle.SCHEME_CKKS, N, **how)
    assert g.moduli == o.moduli
    return g, o


def f64(buf, shape):
    return buf.download().view(np.float64)[:int(np.prod(shape))].reshape(shape)


# ---- the codec -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", co.CKKS_ENCODE_N)
def test_the_complex_codec_against_the_host_client(be, oracle, N):
    g, o = contexts(be, oracle, N, {"bit_sizes": co.CKKS_ENCODE_CHAIN, "sec128": False})
    h = cx.ComplexHost(co.host_sim(), N, co.CKKS_ENCODE_CHAIN)
    fixture = cx.load_fixture()
    L, half, n, scale = g.L, N // 2, 3, cx.SCALE
    try:
        for count in cx.counts(N):
            rng = np.random.default_rng(N + count)
            rows = np.stack([cx.complex_input(N, count)] + [rng.uniform(-0.7, 0.7, count) + 1j * rng.uniform(-0.7, 0.7, count) for _ in range(n - 1)])
            d_vals = g.to_device(np.ascontiguousarray(rows).view(np.float64).view(np.uint64))
            plain = sentinelled(g, n * L * N, N)
            g.ckks_encode_complex(n, d_vals, count, scale, At(plain, N))
            got = inner_of(plain, N, "d_plain").reshape(n, L, N)
            for r in range(n):
                assert np.array_equal(got[r], h.ckks_encode_complex(rows[r], scale)), (count, r)
            case = next(c for c in fixture["encode"] if c["N"] == N and c["count"] == count)
            cx.check_encode_case(fixture, case, co.coeffs_from_plain(o, got[0]), "device")
            # im = +0.0: the real encoder's bits
            re = np.ascontiguousarray(rows.real)
            d_re, d_rc = g.to_device(re.view(np.uint64)), g.to_device(np.ascontiguousarray(re.astype(np.complex128)).view(np.float64).view(np.uint64))
            p_re, p_rc = g.alloc(n * L * N), g.alloc(n * L * N)
            g.ckks_encode(n, d_re, count, scale, p_re)
            g.ckks_encode_complex(n, d_rc, count, scale, p_rc)
            assert np.array_equal(p_re.download(), p_rc.download()), count
            # decode: the pairs are the host's, the re parts he355_ckks_decode's, the round trip inside N / scale
            d_plain = g.to_device(got)
            out_c, out_r = sentinelled(g, n * half * 2, N), g.alloc(n * half)
            g.ckks_decode_complex(L, n, d_plain, scale, At(out_c, N))
            g.ckks_decode(L, n, d_plain, scale, out_r)
            back = inner_of(out_c, N, "d_out").view(np.float64).reshape(n, half, 2)
            assert np.array_equal(back[:, :, 0], f64(out_r, (n, half))), count
            assert np.array_equal(d_plain.download((n, L, N)), got), "d_plain"
            for r in range(n):
                assert np.array_equal(back[r].reshape(-1).view(np.complex128), h.ckks_decode_complex(got[r], scale)), (count, r)
            z = back.reshape(n, -1).view(np.complex128)
            assert float(np.max(np.abs(z[:, :count] - rows))) <= N / scale and float(np.max(np.abs(z[:, count:]), initial=0.0)) <= N / scale, count
            ranges = [(0, 3), (half - 2, 2)]
            out_s = sentinelled(g, n * 5 * 2, N)
            g.ckks_decode_complex_slots(L, n, d_plain, scale, ranges, At(out_s, N))
            sl = inner_of(out_s, N, "slots").view(np.float64).reshape(n, 5, 2)
            assert np.array_equal(sl, np.concatenate([back[:, f:f + c] for f, c in ranges], axis=1)), count
            for b in (d_vals, plain, d_re, d_rc, p_re, p_rc, d_plain, out_c, out_r, out_s):
                b.free()
    finally:
        h.close()
        g.close()


@pytest.mark.parametrize("chain", list(cx.DECODE_LEVELS))
def test_the_complex_decode_against_the_exact_slots(be, oracle, chain):
    N, bits, _ = co.DECODE_CHAINS[chain]
    g, o = contexts(be, oracle, N, {"bit_sizes": bits, "sec128": False})
    by_id = {c["id"]: c for c in cx.load_fixture()["decode"]}
    half = N // 2
    try:
        for L, fam, plain, cases in co.decode_operands(o, chain, co.load_fixture()):
            if L not in cx.DECODE_LEVELS[chain]:
                continue
            d_plain = g.to_device(plain)
            for case in cases:
                out = g.alloc(half * 2)
                g.ckks_decode_complex(L, 1, d_plain, float.fromhex(case["scale"]), out)
                z = f64(out, (half, 2))
                co.check_decode_case(case, z[:, 0], "device")
                cx.check_decode_case(by_id[case["id"]], case["positions"], z[:, 1], "device")
                out.free()
            d_plain.free()
    finally:
        g.close()


# ---- the combination -------------------------------------------------------------------------------------------------------------------
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


def run_combine(g, L, size, slabs, order, scalars, const, real=False):
    """slabs: host arrays [n][size][L_t][N]; order: the slab of each term (a slab named twice is the same device pointer).  -> [n][size][L][N]"""
    N = g.N
    bufs = [g.to_device(t) for t in slabs]
    n = slabs[0].shape[0]
    d_out = sentinelled(g, n * size * L * N, N)
    terms = [(bufs[k], slabs[k].shape[2]) for k in order]
    (g.combine_scalars if real else g.combine_scalars_complex)(L, size, n, terms, scalars, At(d_out, N), const)
    got = inner_of(d_out, N, "d_out").reshape(n, size, L, N)
    for b, t in zip(bufs, slabs):
        assert np.array_equal(b.download(t.shape), t), "a term changed"
        b.free()
    d_out.free()
    return got


def grouped(order, scalars, L, k):
    """the integer sums of the scalar pairs of the terms that read slab k: the definition's sum, regrouped (no reduction)"""
    return [[sum(int(scalars[t][h][i]) for t in range(len(order)) if order[t] == k) for i in range(L)] for h in range(2)]


def test_combine_against_the_definition(cctx):
    g, o, rng = cctx
    q = o.moduli
    L = g.L - 1  # the second slab lies one level higher and is read with its own stride
    draw = lambda: [int(rng.integers(0, q[i])) for i in range(L)]
    top = [q[i] - 1 for i in range(L)]
    for size, n in ((2, 1), (3, 3)):
        slabs = [rand_cts(o, rng, n, L, size), rand_cts(o, rng, n, L + 1, size)]
        for terms in (1, 2, 257):
            order = [1] if terms == 1 else [0, 1] + [t % 2 for t in range(terms - 2)]  # a repeated pointer from the third term on
            scalars = [[top, draw()] if t % 2 == 0 else [draw(), top] for t in range(terms)]
            for const in (None, [top, draw()]):
                g.poly_stats(reset=True)
                got = run_combine(g, L, size, slabs, order, scalars, const)
                st = g.poly_stats()
                assert st["complex_combinations"] == 1 and st["combinations"] == 0 and st["calls"] == 0, st
                used = sorted(set(order))
                for c in range(n):
                    want = cref.combine(q, L, [slabs[k][c] for k in used], [grouped(order, scalars, L, k) for k in used], const)
                    assert np.array_equal(got[c], want), (size, n, terms, const is not None, "ciphertext", c)
    # 257 terms of (q - 1)^2 with a constant of q - 1: one fold of the 128-bit sums under the 60-bit primes, in both halves
    N = g.N
    full = np.stack([np.stack([np.stack([np.full(N, q[i] - 1, dtype=np.uint64) for i in range(L)])] * 2)])
    got = run_combine(g, L, 2, [full], [0] * 257, [[top, top]] * 257, [top, top])
    for i in range(L):
        assert (got[0, 0, i] == np.uint64((257 * (q[i] - 1) ** 2 + q[i] - 1) % q[i])).all() and (got[0, 1, i] == np.uint64((257 * (q[i] - 1) ** 2) % q[i])).all(), i


def test_combine_equals_multiply_plain_by_a_plus_bj_and_add_on_the_device(cctx):
    g, o, rng = cctx
    q = o.moduli
    L, N, n = g.L, g.N, 3
    a, b = rand_cts(o, rng, n, L, 2), rand_cts(o, rng, n, L, 2)
    va, vb = (2.0 ** 40 * 0.37, -(2.0 ** 40) * 0.81), (-12345.0, 2.0 ** 58)
    pairs = [g.ckks_complex_scalar_residues(L, *va), g.ckks_complex_scalar_residues(L, *vb)]
    assert pairs == [cref.scalar_residues(q, cref.units(o, L), L, *v) for v in (va, vb)]
    got = run_combine(g, L, 2, [a, b], [0, 1], pairs, None)
    da, db, pa, pb = g.to_device(a), g.to_device(b), g.to_device(cref.scalar_plain(o, L, *va)), g.to_device(cref.scalar_plain(o, L, *vb))
    ta, tb = g.alloc(a.size), g.alloc(a.size)
    one = g.outer(0, n, 0, 1)  # ciphertext r, the one plaintext
    g.multiply_plain(L, 2, n, da, pa, one, ta)
    g.multiply_plain(L, 2, n, db, pb, one, tb)
    g.add(L, 2, n, ta, tb, g.pairwise(), ta)
    assert np.array_equal(ta.download(a.shape), got)
    for x in (da, db, pa, pb, ta, tb):
        x.free()
    # both halves equal: he355_combine_scalars' bits
    sa, sb, cst = [int(rng.integers(0, q[i])) for i in range(L)], [q[i] - 1 for i in range(L)], [int(rng.integers(0, q[i])) for i in range(L)]
    assert np.array_equal(run_combine(g, L, 2, [a, b], [0, 1], [[sa, sa], [sb, sb]], [cst, cst]), run_combine(g, L, 2, [a, b], [0, 1], [sa, sb], cst, real=True))


# ---- the evaluation --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ectx(be, oracle):
    g, o = contexts(be, oracle, 2048, {"bit_sizes": [60, 40, 40, 40, 40, 40, 60], "sec128": False})
    rng = np.random.default_rng(2048)
    rk = o.random_kswitch_key(rng)
    g.set_relin_key(rk)
    yield g, o, rng, rk, 2.0 ** 40
    g.close()


def run_eval(g, L, cts, coeffs, log_baby, scale, L_out, real=False):
    n, N = len(cts), g.N
    d_in = g.to_device(cts)
    d_out = sentinelled(g, n * 2 * L_out * N, N)
    (g.ckks_eval_poly if real else g.ckks_eval_poly_complex)(L, n, d_in, coeffs, log_baby, scale, scale, At(d_out, N))
    got = inner_of(d_out, N, "d_out").reshape(n, 2, L_out, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    d_in.free()
    d_out.free()
    return got


@pytest.mark.parametrize("log_baby", [1, 2])
@pytest.mark.parametrize("poly", ["cubic", "septic"])
def test_eval_poly_complex_against_the_reference(ectx, poly, log_baby):
    g, o, rng, rk, scale = ectx
    coeffs, L, n = {"cubic": CUBIC, "septic": SEPTIC}[poly], g.L, 3
    g.set_chunk(2)
    try:
        cts = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
        pl = g.ckks_eval_poly_complex_plan(L, coeffs, log_baby, scale, scale, n)
        assert pl["chunks"] == 2
        g.poly_stats(reset=True)
        got = run_eval(g, L, cts, coeffs, log_baby, scale, pl["L_out"])
        st = g.poly_stats()
        assert st["calls"] == 1 and st["chunks"] == 2 and st["combinations"] == 0 and st["complex_combinations"] == pl["combinations"] * 2, (st, pl)
        for k in ("products", "rescales", "drops", "adds"):
            assert st[k] == pl[k] * 2, (k, st, pl)
        for c in range(n):
            want, ev = cref.eval_poly(o, cts[c], coeffs, log_baby, scale, scale, rk, composed=True)
            assert ev.counters() == {k: pl[k] for k in ev.counters()}
            assert np.array_equal(got[c], want), (poly, log_baby, "ciphertext", c)
    finally:
        g.set_chunk(1024)


def test_zero_imaginary_parts_give_the_real_call(ectx):
    g, o, rng, rk, scale = ectx
    L = g.L
    cts = np.stack([o.random_poly(rng, L, 2) for _ in range(2)])
    for coeffs, log_baby in (([0.5, 0.15012, 0.0, -0.0015930078125], 1), ([0.0, 0.31831, 0.0, -0.10610, 0.0, 0.06366, 0.0, -0.04547], 2), ([1.0, 0.0, 0.0, 0.0, 0.5], 1)):
        pl = g.ckks_eval_poly_plan(L, coeffs, log_baby, scale, scale, 2)
        want = run_eval(g, L, cts, coeffs, log_baby, scale, pl["L_out"], real=True)
        assert np.array_equal(run_eval(g, L, cts, [complex(c) for c in coeffs], log_baby, scale, pl["L_out"]), want), coeffs


# ---- two compositions with real keys -----------------------------------------------------------------------------------------------------
def disc(rng, count):
    return rng.uniform(-0.7, 0.7, count) + 1j * rng.uniform(-0.7, 0.7, count)


def test_real_and_imaginary_parts_of_an_encrypted_complex_vector(be, oracle):
    N, scale, seed = 1024, 2.0 ** 40, 500
    g, o = contexts(be, oracle, N, {"bit_sizes": BITS, "sec128": False})
    L, conj = g.L, 2 * N - 1
    z = disc(np.random.default_rng(seed), N // 2)
    sk = o.keygen_secret(seed)
    pk, gk = o.keygen_public(sk, seed + 1), o.keygen_galois(sk, conj, seed + 2)
    g.set_galois_key(conj, gk)
    # the ciphertext from the device's own complex encoder, encrypted by the oracle
    d_vals, d_pt = g.to_device(np.ascontiguousarray(z).view(np.float64).view(np.uint64)), g.alloc(L * N)
    g.ckks_encode_complex(1, d_vals, N // 2, scale, d_pt)
    x = o.encrypt(pk, d_pt.download((L, N)), seed + 3)
    W = float(o.moduli[L - 1])  # the weight the rescale takes away again
    parts = {"re": ((W / 2, 0.0), (W / 2, 0.0), z.real), "im": ((0.0, -W / 2), (0.0, W / 2), z.imag)}  # (z + conj z) / 2 and -i (z - conj z) / 2
    d_x, d_c = g.to_device(x[None]), g.alloc(2 * L * N)
    g.apply_galois(L, 1, d_x, conj, d_c)
    xc = o.apply_galois(x, conj, gk)
    assert np.array_equal(d_c.download((2, L, N)), xc)
    dec = lambda ct: oracle.ckks_decode(o, o.decrypt_phase(ct, sk), scale)
    for name, (on_x, on_c, want) in parts.items():
        pairs = [g.ckks_complex_scalar_residues(L, *on_x), g.ckks_complex_scalar_residues(L, *on_c)]
        d_sum, d_out = g.alloc(2 * L * N), g.alloc(2 * (L - 1) * N)
        g.combine_scalars_complex(L, 2, 1, [(d_x, L), (d_c, L)], pairs, d_sum)
        g.rescale(L, 2, 1, d_sum, d_out)
        got = d_out.download((2, L - 1, N))
        assert np.array_equal(got, o.rescale(cref.combine(o.moduli, L, [x, xc], pairs))), name
        # the reference run: the oracle's multiply_plain by the encoded constant vectors, add, rescale -- on the same ciphertexts
        enc = lambda v: oracle.ckks_encode(o, np.full(N // 2, complex(*v) / W), W)
        ref_ct = o.rescale(o.add(o.multiply_plain(x, enc(on_x)), o.multiply_plain(xc, enc(on_c))))
        err, err_ref = float(np.max(np.abs(dec(got) - want))), float(np.max(np.abs(dec(ref_ct) - want)))
        print(f"{name} part: device {err:.3e}  reference run {err_ref:.3e}")
        assert err_ref < 1e-6 and err <= 2.0 * err_ref, (name, err, err_ref)  # (2: the second rounding, B, and J's sqrt 2 on the noise)
        d_sum.free()
        d_out.free()
    g.close()


def test_a_complex_banded_matrix_two_by_two(be, oracle):
    N, scale, seed = 1024, 2.0 ** 30, 600
    g, o = contexts(be, oracle, N, {"bit_sizes": [50, 40, 40, 50], "sec128": False})
    L, n = g.L, N // 2
    baby, giant = [0, 1], [0, 2]
    sk = o.keygen_secret(seed)
    pk = o.keygen_public(sk, seed + 1)
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), seed + 10 + s) for s in (1, 2)}
    for e, k in keys.items():
        g.set_galois_key(e, k)
    rng = np.random.default_rng(seed)
    x, diags = disc(rng, n), np.stack([disc(rng, n) for _ in range(4)])
    want = _diagonals(n, 4, diags) @ x
    ct = o.encrypt(pk, oracle.ckks_encode(o, x, scale), seed + 2)
    split = np.stack([v for row in bsgs.split_diagonals(diags, baby, giant, lambda v, s: np.roll(v, -s)) for v in row])
    d_vals, d_pt, d_qp, d_bad = g.to_device(np.ascontiguousarray(split).view(np.float64).view(np.uint64)), g.alloc(4 * L * N), g.alloc(4 * (L + 1) * N), g.alloc(1)
    g.ckks_encode_complex(4, d_vals, n, scale, d_pt)
    g.plain_extend_special(L, 4, d_pt, d_qp, d_bad)
    assert int(d_bad.download()[0]) == 0
    d_in, d_out = g.to_device(ct[None]), g.alloc(2 * L * N)
    g.linear_transform_bsgs(L, 1, d_in, baby, giant, d_qp, d_out)
    got = d_out.download((2, L, N))
    assert np.array_equal(got, bsgs.linear_transform_bsgs(o, ct[None], baby, giant, keys, d_qp.download((2, 2, L + 1, N)))[0])
    # the reference run: the same transform on the oracle (tests/linear_transform_bsgs_ref.py) with the ORACLE's complex encoding of the
    # diagonals, extended by the reference's extend_special.  The two runs share ciphertext, keys and route and differ in the encoders'
    # roundings alone (each within a unit per coefficient of the exact value: tests/test_ckks_complex_core_cpu.py), far below the key-switch
    # noise; the cap is the one the real 4 x 4 case is held to.
    ref_qp = np.stack([lazy.extend_special(o, oracle.ckks_encode(o, v, scale))[0] for v in split]).reshape(2, 2, L + 1, N)
    acc = bsgs.linear_transform_bsgs(o, ct[None], baby, giant, keys, ref_qp)[0]
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    err, err_ref = float(np.max(np.abs(dec(got) - want))), float(np.max(np.abs(dec(acc) - want)))
    print(f"complex 4 diagonals: bsgs 2x2 {err:.3e}  reference run {err_ref:.3e}")
    assert err_ref < 1e-2 and err <= CKKS_RATIO_CAP * err_ref, (err, err_ref)
    g.close()
