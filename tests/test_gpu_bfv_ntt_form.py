"""GPU parity of the NTT-form BFV operands (he355_bfv_transform_to_ntt / transform_from_ntt, he355_bfv_plain_to_ntt,
he355_bfv_multiply_plain_ntt, he355_bfv_multiply_plain_accumulate), bit-exact (np.array_equal, no tolerance) against the oracle's
transforms and Python integers, on the CONFIGS and the three random chains of tests/test_gpu_bfv_levels.py:

* transforms  : to_ntt equals oracle.ntt per polynomial, from_ntt(to_ntt(x)) == x; in place and apart, sizes 1..3, every L, n = 1, 5, 300;
* plain_to_ntt: oracle.ntt(i, lift(m) mod q_i), the lift in Python integers; monomial, zero, -X^k and full-range plaintexts;
* multiply    : the pointwise product in Python integers; from_ntt(multiply_plain_ntt(to_ntt(ct), plain_to_ntt(m))) bit-equal to
                he355_bfv_multiply_plain(ct, m), outer-product and pairwise;
* accumulate  : the Python-integer sum of per-prime products of oracle.ntt values AND the unfused device loop (multiply_plain_ntt + add),
                shapes (1,1,1), (1,1,7), (3,2,5), (1,5,16), (5,1,16), natural and transposed non-unit strides, sizes 1..3, every L;
                at N = 1024 under 60-bit primes inner = 255, 256, 257, 600 with coefficients forced to q - 1 in both operands (a full
                128-bit run, and the cut between runs);
* semantic    : Dec(from_ntt(sum_k to_ntt(Enc(x_k)) (.) plain_to_ntt(encode(p_kj)))) = sum_k x_k p_kj mod t slot-wise with real keys, by
                the oracle's decryption and by he355_decrypt + he355_bfv_decode, with noise budget left;
* ordering    : an asynchronous producer (he355_add into an operand) immediately followed by each new call, small chunks, dual stream;
* refusals    : overlaps, inner == 0, size 0 or 4, L out of range: HE355_E_INVALID_ARGS and the outputs untouched;
* no raw hipMalloc / hipFree in a second call."""

import numpy as np
import pytest

from bfv_gpu_helpers import ALL, SENT, At, be, lift, pair, plains, rand_cts, refused  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 1, 7), (3, 2, 5), (1, 5, 16), (5, 1, 16)]


def ntt_cts(o, cts):
    """oracle.ntt of every polynomial of [n][size][L][N]"""
    out = np.empty_like(cts)
    for r in range(cts.shape[0]):
        for k in range(cts.shape[1]):
            for i in range(cts.shape[2]):
                out[r, k, i] = o.ntt(i, cts[r, k, i])
    return out


def ntt_plains(o, pls, L):
    """[n][L][N]: oracle.ntt(i, lift(m) mod q_i), the lift in Python integers"""
    out = np.empty((pls.shape[0], L, pls.shape[1]), dtype=np.uint64)
    for j in range(pls.shape[0]):
        lm = lift(o, pls[j], L)
        for i in range(L):
            out[j, i] = o.ntt(i, lm[i])
    return out


def exact_sum(A, B, q):
    """sum_k A[k] * B[k] mod q, exact: A, B uint64 [inner][...] below 2^63.  The operands are cut in 21-bit limbs, so a limb product is below
    2^42 and the sums of up to three of them over `inner` < 2^20 terms stay below 2^64 in uint64; the five partial sums are then put
    together and reduced in Python integers."""
    assert A.shape[0] < (1 << 20)
    m, s = np.uint64((1 << 21) - 1), np.uint64(21)
    a = [A & m, (A >> s) & m, A >> (s + s)]
    b = [B & m, (B >> s) & m, B >> (s + s)]
    tot = 0
    for w in range(5):
        part = sum((a[u] * b[w - u]).sum(axis=0, dtype=np.uint64) for u in range(3) if 0 <= w - u < 3)
        tot = tot + (part.astype(object) << (21 * w))
    return (tot % q).astype(np.uint64)


def test_exact_sum_is_the_python_integer_sum():
    rng = np.random.default_rng(1)
    for q in ((1 << 60) - 93, (1 << 61) - 1, (1 << 40) - 87):
        A = rng.integers(0, q, (37, 64), dtype=np.uint64)
        B = rng.integers(0, q, (37, 64), dtype=np.uint64)
        A[:, 0] = B[:, 0] = q - 1
        want = [sum(int(A[k, c]) * int(B[k, c]) for k in range(37)) % q for c in range(64)]
        assert exact_sum(A, B, q).tolist() == want


def edged_cts(o, rng, n, L, size):
    c = rand_cts(o, rng, n, L, size)
    c[0, 0, :, :4] = 0
    for i, q in enumerate(o.moduli[:L]):
        c[0, 0, i, 4:8] = q - 1
    return c


@pytest.mark.parametrize("name", list(ALL))
def test_transforms(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(21)
    for L in range(1, g.L + 1):
        for size in (1, 2, 3):
            base = edged_cts(o, rng, 7, L, size)
            want = ntt_cts(o, base)
            for n in (1, 5, 300):
                idx = np.arange(n) % 7
                src = g.to_device(base[idx])
                out = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
                g.bfv_transform_to_ntt(L, size, n, src, out)  # apart
                assert np.array_equal(out.download((n, size, L, N)), want[idx]), (name, L, size, n, "to_ntt apart")
                assert np.array_equal(src.download((n, size, L, N)), base[idx])
                if n < 300:
                    back = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
                    g.bfv_transform_from_ntt(L, size, n, out, back)  # apart
                    assert np.array_equal(back.download((n, size, L, N)), base[idx]), (name, L, size, n, "from_ntt apart")
                    g.bfv_transform_to_ntt(L, size, n, src, src)  # in place
                    assert np.array_equal(src.download((n, size, L, N)), want[idx]), (name, L, size, n, "to_ntt in place")
                    back.free()
                g.bfv_transform_from_ntt(L, size, n, out, out)  # in place
                assert np.array_equal(out.download((n, size, L, N)), base[idx]), (name, L, size, n, "from_ntt in place")
                src.free()
                out.free()
    # n == 0 touches nothing; refusals leave the output as it was
    L, size, n = g.L, 2, 3
    per = size * L * N
    src = g.to_device(rand_cts(o, rng, n, L, size))
    out = g.to_device(np.full((n + 1) * per, SENT, dtype=np.uint64))
    for f in (g.bfv_transform_to_ntt, g.bfv_transform_from_ntt):
        f(L, size, 0, src, out)
        refused(be, lambda: f(L, 0, n, src, out))
        refused(be, lambda: f(L, 4, n, src, out))
        refused(be, lambda: f(0, size, n, src, out))
        refused(be, lambda: f(g.L + 1, size, n, src, out))
        refused(be, lambda: f(L, size, n, out, At(out, per)))       # shifted by one ciphertext: neither in place nor apart
        refused(be, lambda: f(L, size, n, At(out, N), out))
    assert (out.download() == SENT).all()
    g.close()


@pytest.mark.parametrize("name", list(ALL))
def test_plain_to_ntt(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(22)
    pls = plains(o, rng, 6, N)
    pls[2, :6] = [0, 1, o.t // 2, (o.t + 1) // 2, o.t - 1, 2]
    dp = g.to_device(pls)
    for L in range(1, g.L + 1):
        out = g.to_device(np.full(6 * L * N, SENT, dtype=np.uint64))
        g.bfv_plain_to_ntt(L, 6, dp, out)
        got = out.download((6, L, N))
        assert np.array_equal(got, ntt_plains(o, pls, L)), (name, L)
        assert not got[1].any()  # the zero plaintext
        out.free()
    L = g.L
    out = g.to_device(np.full(6 * L * N, SENT, dtype=np.uint64))
    g.bfv_plain_to_ntt(L, 0, dp, out)
    refused(be, lambda: g.bfv_plain_to_ntt(0, 6, dp, out))
    refused(be, lambda: g.bfv_plain_to_ntt(g.L + 1, 6, dp, out))
    refused(be, lambda: g.bfv_plain_to_ntt(L, 2, out, out))
    refused(be, lambda: g.bfv_plain_to_ntt(L, 2, At(out, N), out))
    assert (out.download() == SENT).all()
    assert np.array_equal(dp.download((6, N)), pls)
    g.close()


def pointwise(o, ct, pt):
    """[size][L][N] x [L][N]: the product per residue in Python integers"""
    out = np.empty_like(ct)
    for i in range(ct.shape[1]):
        out[:, i] = ((ct[:, i].astype(object) * pt[i].astype(object)) % o.moduli[i]).astype(np.uint64)
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_multiply_plain_ntt(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(23)
    for L in range(1, g.L + 1):
        for size in (1, 2, 3):
            cts = edged_cts(o, rng, 8, L, size)                      # NTT-form operands are residues like any others
            pts = np.stack([o.random_poly(rng, L, 1)[0] for _ in range(8)])
            pts[1] = 0
            for i, q in enumerate(o.moduli[:L]):
                pts[0, i, :8] = q - 1
            dc, dp = g.to_device(cts), g.to_device(pts)
            for n, ix, ia, ib in ((6, be.Context.outer(1, 3, 2, 2), lambda r: 1 + r // 2, lambda r: 2 + r % 2),
                                  (8, be.Context.pairwise(0, 0), lambda r: r, lambda r: r)):
                out = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
                g.bfv_multiply_plain_ntt(L, size, n, dc, dp, ix, out)
                got = out.download((n, size, L, N))
                for r in range(n):
                    assert np.array_equal(got[r], pointwise(o, cts[ia(r)], pts[ib(r)])), (name, L, size, n, r)
                out.free()
            # in place: pairwise, and one plaintext for every ciphertext (b1 == 1)
            w = g.to_device(cts)
            g.bfv_multiply_plain_ntt(L, size, 8, w, dp, be.Context.pairwise(0, 0), w)
            got = w.download((8, size, L, N))
            for r in range(8):
                assert np.array_equal(got[r], pointwise(o, cts[r], pts[r])), (name, L, size, r)
            w.upload(cts)
            g.bfv_multiply_plain_ntt(L, size, 8, w, dp, be.Context.outer(0, 8, 3, 1), w)
            got = w.download((8, size, L, N))
            for r in range(8):
                assert np.array_equal(got[r], pointwise(o, cts[r], pts[3])), (name, L, size, r)
            # refused: in place when a ciphertext serves two results, a shifted overlap, an output over the plaintexts; size, level
            w.upload(cts)
            v = g.to_device(pts)
            refused(be, lambda: g.bfv_multiply_plain_ntt(L, size, 4, w, dp, be.Context.outer(0, 2, 0, 2), w))
            refused(be, lambda: g.bfv_multiply_plain_ntt(L, size, 3, w, dp, be.Context.pairwise(1, 0), w))
            refused(be, lambda: g.bfv_multiply_plain_ntt(L, 1, 1, dc, v, be.Context.pairwise(), v))
            refused(be, lambda: g.bfv_multiply_plain_ntt(L, 0, 1, dc, dp, be.Context.pairwise(), w))
            refused(be, lambda: g.bfv_multiply_plain_ntt(L, 4, 1, dc, dp, be.Context.pairwise(), w))
            refused(be, lambda: g.bfv_multiply_plain_ntt(g.L + 1, size, 1, dc, dp, be.Context.pairwise(), w))
            refused(be, lambda: g.bfv_multiply_plain_ntt(0, size, 1, dc, dp, be.Context.pairwise(), w))
            assert np.array_equal(w.download((8, size, L, N)), cts) and np.array_equal(v.download((8, L, N)), pts)
            for b in (dc, dp, w, v):
                b.free()
    g.close()


@pytest.mark.parametrize("name", list(ALL))
def test_ntt_form_pipeline_equals_coefficient_form_multiply_plain(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(24)
    for L in range(1, g.L + 1):
        for size in (2, 3):
            cts, pls = rand_cts(o, rng, 8, L, size), plains(o, rng, 8, N)
            dc, dp = g.to_device(cts), g.to_device(pls)
            cn, pn = g.alloc(8 * size * L * N), g.alloc(8 * L * N)
            g.bfv_transform_to_ntt(L, size, 8, dc, cn)
            g.bfv_plain_to_ntt(L, 8, dp, pn)
            for n, ix in ((6, be.Context.outer(1, 3, 0, 2)), (8, be.Context.pairwise(0, 0))):
                want, got = g.alloc(n * size * L * N), g.alloc(n * size * L * N)
                g.bfv_multiply_plain(L, size, n, dc, dp, ix, want)
                g.bfv_multiply_plain_ntt(L, size, n, cn, pn, ix, got)
                g.bfv_transform_from_ntt(L, size, n, got, got)
                assert np.array_equal(got.download(), want.download()), (name, L, size, n)
                want.free()
                got.free()
            for b in (dc, dp, cn, pn):
                b.free()
    g.close()


def layouts(rows, cols, inner):
    """(ct_stride_i, ct_stride_k, pt_stride_k, pt_stride_j): row-major, and transposed with gaps (every index still distinct)"""
    return [(inner, 1, cols, 1), (2, 2 * rows + 1, 3, 3 * inner + 2)]


def run_accumulate(be, g, o, L, size, rows, cols, inner, strides, ctn_vals, ptn_vals, tag):
    """ctn_vals [rows][inner][size][L][N], ptn_vals [inner][cols][L][N]: NTT-form values.  The fused call against the Python-integer sum
    and against the unfused device loop; returns the fused result."""
    N = ctn_vals.shape[-1]
    si, sk, pk, pj = strides
    n_ct, n_pt = (inner - 1) * sk + (rows - 1) * si + 1, (inner - 1) * pk + (cols - 1) * pj + 1
    ch = np.full((n_ct, size, L, N), SENT, dtype=np.uint64)
    ph = np.full((n_pt, L, N), SENT, dtype=np.uint64)
    for k in range(inner):
        for i in range(rows):
            ch[i * si + k * sk] = ctn_vals[i, k]
        for j in range(cols):
            ph[k * pk + j * pj] = ptn_vals[k, j]
    dc, dp = g.to_device(ch), g.to_device(ph)
    per = size * L * N
    out = g.to_device(np.full(rows * cols * per, SENT, dtype=np.uint64))
    g.bfv_multiply_plain_accumulate(L, size, rows, cols, inner, dc, si, sk, dp, pk, pj, out)
    got = out.download((rows, cols, size, L, N))
    for i in range(rows):
        for j in range(cols):
            for li, q in enumerate(o.moduli[:L]):
                want = exact_sum(ctn_vals[i, :, :, li], ptn_vals[:, j, None, li], q)  # [inner][size][N] x [inner][1][N]
                assert np.array_equal(got[i, j, :, li], want), (tag, "python integers", i, j, li)
    # the unfused loop on the device: multiply_plain_ntt of one term, add_inplace
    loop, term = g.alloc(rows * cols * per), g.alloc(per)
    pw = be.Context.pairwise()
    for i in range(rows):
        for j in range(cols):
            acc = At(loop, (i * cols + j) * per)
            for k in range(inner):
                g.bfv_multiply_plain_ntt(L, size, 1, At(dc, (i * si + k * sk) * per), At(dp, (k * pk + j * pj) * L * N), pw, acc if k == 0 else term)
                if k:
                    g.add(L, size, 1, acc, term, pw, acc)
    assert np.array_equal(loop.download((rows, cols, size, L, N)), got), (tag, "unfused loop")
    assert np.array_equal(dc.download((n_ct, size, L, N)), ch) and np.array_equal(dp.download((n_pt, L, N)), ph)
    for b in (dc, dp, out, loop, term):
        b.free()
    return got


@pytest.mark.parametrize("name", list(ALL))
def test_multiply_plain_accumulate(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(25)
    # (the ring of tests/shoup_rings.py: the smaller chains walk every level and size against Python integers; at N = 16384 the top level
    # and L = 1 at size 2 keep the case to a few seconds -- every shape and both layouts still run)
    small = name == "n16384_shoup"
    for L in ((1, g.L) if small else range(1, g.L + 1)):
        for size in ((2,) if small else (1, 2, 3)):
            for rows, cols, inner in SHAPES:
                # coefficient-form operands through the oracle's transforms: what to_ntt / plain_to_ntt hand the call
                cts = rand_cts(o, rng, rows * inner, L, size)
                pls = plains(o, rng, inner * cols, N)
                ctn = ntt_cts(o, cts).reshape(rows, inner, size, L, N)
                ptn = ntt_plains(o, pls, L).reshape(inner, cols, L, N)
                lays = layouts(rows, cols, inner)
                for li, strides in enumerate(lays if L == g.L else lays[:1]):
                    run_accumulate(be, g, o, L, size, rows, cols, inner, strides, ctn, ptn, (name, L, size, rows, cols, inner, li))
    g.close()


@pytest.mark.parametrize("bits", [[60, 60, 60], [60, 40, 60]], ids=["60-60-60", "60-40-60"])
def test_accumulate_full_runs_under_60_bit_primes(be, oracle, bits):
    """inner = 255, 256, 257, 600 at N = 1024: 256 terms of (q - 1)^2 fill the 128-bit sum of a 60-bit prime to less than one term of room"""
    N = 1024
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    assert g.moduli == o.moduli and o.moduli[0].bit_length() == 60
    rng = np.random.default_rng(26)
    L, size = g.L, 2
    for inner in (255, 256, 257, 600):
        for rows, cols in ((1, 1), (2, 3)):
            ctn = np.stack([o.random_poly(rng, L, size) for _ in range(rows * inner)]).reshape(rows, inner, size, L, N)
            ptn = np.stack([o.random_poly(rng, L, 1)[0] for _ in range(inner * cols)]).reshape(inner, cols, L, N)
            for i, q in enumerate(o.moduli[:L]):
                ctn[:, :, :, i, :16] = q - 1          # every term of these coefficients is (q - 1)^2 ...
                ptn[:, :, i, :12] = q - 1
                ptn[:, :, i, 12:16] = 0               # ... or 0
                ctn[:, :, :, i, 16:20] = 0
            got = run_accumulate(be, g, o, L, size, rows, cols, inner, (inner, 1, cols, 1), ctn, ptn, (bits, inner, rows, cols))
            for i, q in enumerate(o.moduli[:L]):
                assert (got[:, :, :, i, :12] == inner * (q - 1) ** 2 % q).all() and not got[:, :, :, i, 12:20].any()
    g.close()


@pytest.mark.parametrize("N,bits", [(8192, [60, 40, 60]), (32768, [60, 40, 40, 60])])
def test_semantic_plain_matrix_times_encrypted_vector(be, oracle, N, bits):
    """Dec(from_ntt(sum_k to_ntt(Enc(x_k)) (.) plain_to_ntt(encode(p_kj)))) = sum_k x_k p_kj mod t slot-wise: real keys from the oracle, x and p
    uniform over the full centred range, t of 20 bits, inner = 16; decrypted by the oracle and by he355_decrypt + he355_bfv_decode."""
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    assert g.moduli == o.moduli and g.t == o.t and o.t.bit_length() == 20
    t, L = o.t, g.L
    codec = oracle.BatchCodec(N, t)
    rng = np.random.default_rng(N + 1)
    sk = o.keygen_secret(41)
    pk = o.keygen_public(sk, 42)
    g.set_public_key(pk)
    g.set_secret_key(sk)
    inner, cols = 16, 3
    x = rng.integers(-(t // 2), t // 2 + 1, (inner, N))
    p = rng.integers(-(t // 2), t // 2 + 1, (inner, cols, N))
    want = (x.astype(object)[:, None, :] * p.astype(object)).sum(axis=0) % t
    want = np.where(want > t // 2, want - t, want).astype(np.int64)  # [cols][N]
    enc = lambda v: np.stack([codec.encode(row) for row in v])
    ct, ptn = g.alloc(inner * 2 * L * N), g.alloc(inner * cols * L * N)
    g.encrypt(inner, g.to_device(enc(x)), 51, 0, ct)
    fresh = g.bfv_noise_budget(L, 2, inner, ct)
    g.bfv_transform_to_ntt(L, 2, inner, ct, ct)
    g.bfv_plain_to_ntt(L, inner * cols, g.to_device(enc(p.reshape(inner * cols, N))), ptn)
    res = g.alloc(cols * 2 * L * N)
    g.bfv_multiply_plain_accumulate(L, 2, 1, cols, inner, ct, 0, 1, ptn, cols, 1, res)
    g.bfv_transform_from_ntt(L, 2, cols, res, res)
    budget = g.bfv_noise_budget(L, 2, cols, res)
    print(f"noise budget N={N} {bits}: fresh {fresh.min()}..{fresh.max()} bits, after the inner product of {inner} terms {budget.tolist()} bits")
    assert (budget > 0).all() and (budget < fresh.min()).all()
    cts = res.download((cols, 2, L, N))
    dec, vals = g.alloc(cols * N), g.alloc(cols * N)
    g.decrypt(L, 2, cols, res, dec)
    g.bfv_decode(cols, dec, vals)
    got_dev = vals.download().view(np.int64).reshape(cols, N)
    for j in range(cols):
        v = codec.decode(o.bfv_decode_phase(o.decrypt_phase(cts[j], sk)))
        v = np.where(v > t // 2, v - t, v)
        assert np.array_equal(v, want[j]), (j, "oracle decryption")
        assert np.array_equal(got_dev[j], want[j]), (j, "device decryption")
    g.close()


@pytest.mark.parametrize("name", ["n8192_default", "n1024", "n32768_d3"])
def test_async_producer_then_each_call(be, oracle, name):
    """The operand is still being written by he355_add (asynchronous, first stream) when each new call is issued, with small chunks and the
    dual stream on: whatever stream a call uses has to be ordered behind the producer."""
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(27)
    L, size, n = g.L, 2, 8
    g.set_dual_stream(True)
    g.set_chunk(3)
    x, y = rand_cts(o, rng, n, L), rand_cts(o, rng, n, L)
    a_host = np.stack([o.add(x[r], y[r]) for r in range(n)])
    a_ntt = ntt_cts(o, a_host)
    px, py = (np.stack([o.random_poly(rng, L, 1)[0] for _ in range(n)]) for _ in range(2))  # two halves of the plaintext operands
    p_host = np.stack([o.add(px[r][None], py[r][None])[0] for r in range(n)])
    pls = plains(o, rng, n, N)
    dx, dy, dpx, dpy, dpl = g.to_device(x), g.to_device(y), g.to_device(px), g.to_device(py), g.to_device(pls)
    pw = be.Context.pairwise()
    rows, cols, inner = 2, 2, 4  # a: [rows][inner] ciphertexts, p: [inner][cols] plaintexts
    for rep in range(3):
        a, p = g.to_device(np.zeros_like(x)), g.to_device(np.zeros_like(px))
        o_to, o_from, o_mp, o_acc, o_pt = [g.alloc(n * 2 * L * N) for _ in range(4)] + [g.alloc(n * L * N)]
        g.sync()
        g.add(L, 2, n, dx, dy, pw, a)
        g.bfv_transform_to_ntt(L, size, n, a, o_to)
        g.add(L, 2, n, dx, dy, pw, a)
        g.bfv_transform_from_ntt(L, size, n, a, o_from)
        g.add(L, 2, n, dx, dy, pw, a)
        g.add(L, 1, n, dpx, dpy, pw, p)
        g.bfv_multiply_plain_ntt(L, size, n, a, p, pw, o_mp)
        g.add(L, 2, n, dx, dy, pw, a)
        g.add(L, 1, n, dpx, dpy, pw, p)
        g.bfv_multiply_plain_accumulate(L, size, rows, cols, inner, a, inner, 1, p, cols, 1, o_acc)
        q_plain = g.to_device(np.zeros_like(pls))
        dpl.copy_into(q_plain)  # asynchronous device-to-device copy on the context's stream: the producer of the plaintexts
        g.bfv_plain_to_ntt(L, n, q_plain, o_pt)
        assert np.array_equal(o_to.download((n, 2, L, N)), a_ntt), rep
        back = o_from.download((n, 2, L, N))
        for r in range(n):
            for k in range(2):
                for i in range(L):
                    assert np.array_equal(back[r, k, i], o.intt(i, a_host[r, k, i])), (rep, r, k, i)
        mp = o_mp.download((n, 2, L, N))
        for r in range(n):
            assert np.array_equal(mp[r], pointwise(o, a_host[r], p_host[r])), (rep, r)
        acc = o_acc.download((n, 2, L, N))[:rows * cols].reshape(rows, cols, 2, L, N)
        av, pv = a_host.reshape(rows, inner, 2, L, N), p_host.reshape(inner, cols, L, N)
        for i in range(rows):
            for j in range(cols):
                for li, q in enumerate(o.moduli[:L]):
                    assert np.array_equal(acc[i, j, :, li], exact_sum(av[i, :, :, li], pv[:, j, None, li], q)), (rep, i, j, li)
        assert np.array_equal(o_pt.download((n, L, N)), ntt_plains(o, pls, L)), rep
        for b in (a, p, o_to, o_from, o_mp, o_acc, o_pt, q_plain):
            b.free()
    g.close()


def test_accumulate_refusals_leave_the_output_untouched(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    rng = np.random.default_rng(28)
    L, size = g.L, 2
    per = size * L * N
    cts = rand_cts(o, rng, 6, L, size)
    pts = np.stack([o.random_poly(rng, L, 1)[0] for _ in range(6)])
    dc, dp = g.to_device(cts), g.to_device(pts)
    out = g.to_device(np.full(4 * per, SENT, dtype=np.uint64))
    call = lambda L_=L, size_=size, rows=2, cols=2, inner=3, c=dc, p=dp, o_=out: g.bfv_multiply_plain_accumulate(L_, size_, rows, cols, inner, c, 3, 1, p, 2, 1, o_)
    refused(be, lambda: call(inner=0))
    refused(be, lambda: call(inner=1 << 31))
    refused(be, lambda: call(size_=0))
    refused(be, lambda: call(size_=4))
    refused(be, lambda: call(L_=0))
    refused(be, lambda: call(L_=g.L + 1))
    call(rows=0)   # rows * cols == 0: nothing is launched, nothing is written
    call(cols=0)
    assert (out.download() == SENT).all()
    # the output over an operand: the ciphertexts, their last one only, the plaintexts
    refused(be, lambda: call(o_=dc))
    refused(be, lambda: call(o_=At(dc, 2 * per), rows=1, cols=1))   # (inner = 3: ciphertexts 0, 1, 2 are read)
    refused(be, lambda: call(o_=dp, size_=1, rows=1, cols=1))
    refused(be, lambda: call(c=At(out, N)))
    assert np.array_equal(dc.download((6, size, L, N)), cts) and np.array_equal(dp.download((6, L, N)), pts)
    assert (out.download() == SENT).all()
    g.close()


def test_second_call_makes_no_raw_allocation(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n8192_default")
    rng = np.random.default_rng(29)
    L, n = g.L, 8
    g.set_chunk(3)
    dc, dp = g.to_device(rand_cts(o, rng, n, L)), g.to_device(plains(o, rng, n, N))
    cn, pn, out, acc = g.alloc(n * 2 * L * N), g.alloc(n * L * N), g.alloc(n * 2 * L * N), g.alloc(4 * 2 * L * N)
    pw = be.Context.pairwise()
    stats = []
    for _ in range(3):
        g.bfv_transform_to_ntt(L, 2, n, dc, cn)
        g.bfv_plain_to_ntt(L, n, dp, pn)
        g.bfv_multiply_plain_ntt(L, 2, n, cn, pn, pw, out)
        g.bfv_multiply_plain_accumulate(L, 2, 2, 2, 4, cn, 4, 1, pn, 2, 1, acc)
        g.bfv_multiply_plain_accumulate(L, 2, 1, 1, 8, cn, 0, 1, pn, 1, 0, acc)
        g.bfv_transform_from_ntt(L, 2, n, out, out)
        g.sync()
        stats.append(g.alloc_stats())
    assert stats[0]["raw_mallocs"] == stats[1]["raw_mallocs"] == stats[2]["raw_mallocs"], stats
    assert stats[0]["raw_frees"] == stats[1]["raw_frees"] == stats[2]["raw_frees"], stats
    g.close()
