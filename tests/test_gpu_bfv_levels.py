"""GPU parity of the BFV level operations (he355_bfv_mod_switch, he355_bfv_add_plain / sub_plain, he355_bfv_multiply_plain), bit-exact
(np.array_equal) against the oracle and Python integers:

* mod_switch  : iterated oracle.mod_switch_coeff (ho_mod_switch_coeff), every (L, L_to), sizes 2 and 3, n = 1, 5, 300;
* add / sub   : oracle.add (Python-integer difference for sub) of the ciphertext with [Delta_L(m), 0, ..], Delta_L(m) = floor((q_L m + floor((t+1)/2)) / t) in Python integers;
* multiply    : (i) per prime, oracle.intt(oracle.ntt(c_k) (.) oracle.ntt(lift(m))) with the pointwise product in Python integers, and
                (ii) at N = 1024 a schoolbook negacyclic convolution in Python integers, no transform at all;
* ordering    : an asynchronous producer (he355_add into the operand) immediately followed by each op, the batch cut over both streams;
* semantic    : Dec(mod_switch_to(L')(Enc(x) (.) p + r)) = x p + r mod t slot-wise at every level, with real keys, by the oracle's decryption
                and by he355_decrypt + he355_bfv_decode;
* no raw hipMalloc in a second call."""
import numpy as np
import pytest

from bfv_gpu_helpers import ALL, SENT, be, lift, pair, plains, rand_cts, refused  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu


def switch_to(o, ct, L_to):
    while ct.shape[1] > L_to:
        ct = o.mod_switch_coeff(ct)
    return ct


def delta(o, m, L):
    """[L][N]: floor((q_L m + floor((t + 1) / 2)) / t) mod q_i in Python integers"""
    t, qs = o.t, o.moduli[:L]
    qL = 1
    for q in qs:
        qL *= q
    d = (qL * m.astype(object) + (t + 1) // 2) // t
    return np.stack([(d % q).astype(np.uint64) for q in qs])


def addsub(o, a, b, sub):
    """a +- b per residue ([size][L][N]); the sum through the oracle, the difference in Python integers"""
    if not sub:
        return o.add(a, b)
    out = np.empty_like(a)
    for i in range(a.shape[1]):
        out[:, i] = ((a[:, i].astype(object) - b[:, i].astype(object)) % o.moduli[i]).astype(np.uint64)
    return out


def mul_plain_transform(o, ct, m):
    """expectation (i): per prime intt(ntt(c_k) (.) ntt(lift(m))), pointwise product in Python integers"""
    size, L, _ = ct.shape
    lm = lift(o, m, L)
    out = np.empty_like(ct)
    for i in range(L):
        q = o.moduli[i]
        pm = o.ntt(i, lm[i]).astype(object)
        for k in range(size):
            out[k, i] = o.intt(i, ((o.ntt(i, ct[k, i]).astype(object) * pm) % q).astype(np.uint64))
    return out


def schoolbook(c, lm, q, js):
    """coefficients js of c * lm in Z_q[X]/(X^N + 1), Python integers"""
    N = len(c)
    cc, ll = [int(v) for v in c], [int(v) for v in lm]
    out = []
    for j in js:
        s = 0
        for a in range(N):
            b = j - a
            s += cc[a] * ll[b] if b >= 0 else -cc[a] * ll[b + N]
        out.append(s % q)
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_mod_switch_every_level_pair(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(11)
    Ltop = g.L
    for L in range(1, Ltop + 1):
        for size in (2, 3):
            base = rand_cts(o, rng, 7, L, size)
            base[0, 0, :, :4] = 0                                   # edges: 0, q - 1 and the values where c_last + floor(q_last / 2) wraps
            for i, q in enumerate(o.moduli[:L]):
                base[0, 0, i, 4:8] = q - 1
                base[0, 1, i, :8] = [q - q // 2 - 1, q - q // 2, q - q // 2 + 1, q // 2, q // 2 + 1, q // 2 - 1, 1, q - 2]
            for n in (1, 5, 300):
                idx = np.arange(n) % 7
                src = g.to_device(base[idx])
                for L_to in range(1, L + 1):
                    want = [switch_to(o, base[k], L_to) for k in range(min(n, 7))]
                    out = g.alloc(n * size * L_to * N)
                    g.bfv_mod_switch(L, L_to, size, n, src, out)
                    got = out.download((n, size, L_to, N))
                    for r in range(n):
                        assert np.array_equal(got[r], want[idx[r]]), (name, L, L_to, size, n, r)
                    if L_to == L:
                        assert np.array_equal(got, base[idx])       # a copy
                    out.free()
                src.free()
    # refusals leave the output as it was
    L, size, n = Ltop, 2, 2
    src = g.to_device(rand_cts(o, rng, n, L, size))
    out = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
    refused(be, lambda: g.bfv_mod_switch(L, 0, size, n, src, out))
    refused(be, lambda: g.bfv_mod_switch(L, L + 1, size, n, src, out))
    refused(be, lambda: g.bfv_mod_switch(Ltop + 1, 1, size, n, src, out))
    refused(be, lambda: g.bfv_mod_switch(0, 0, size, n, src, out))
    refused(be, lambda: g.bfv_mod_switch(L, 1, 4, n, src, out))
    assert (out.download() == SENT).all()
    before = src.download()
    refused(be, lambda: g.bfv_mod_switch(L, 1, size, n, src, src))  # in place
    refused(be, lambda: g.bfv_mod_switch(L, L, size, n, src, src))
    assert np.array_equal(src.download(), before)
    g.close()


@pytest.mark.parametrize("name", list(ALL))
def test_add_sub_plain(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(12)
    for L in range(1, g.L + 1):
        for size in (2, 3):
            zeros = np.zeros((size - 1, L, N), dtype=np.uint64)
            cts, pls = rand_cts(o, rng, 5, L, size), plains(o, rng, 6, N)
            pls[2, :6] = [0, 1, o.t // 2, (o.t + 1) // 2, o.t - 1, 2]
            dm = [np.concatenate([delta(o, pls[j], L)[None], zeros]) for j in range(6)]
            dc, dp = g.to_device(cts), g.to_device(pls)
            for sub in (False, True):
                op = lambda a, b: addsub(o, a, b, sub)
                # outer product 3 x 2 from value indices (1, 2)
                out = g.alloc(6 * size * L * N)
                g.bfv_add_plain(L, size, 6, dc, dp, be.Context.outer(1, 3, 2, 2), out, sub=sub)
                got = out.download((6, size, L, N))
                for r in range(6):
                    assert np.array_equal(got[r], op(cts[1 + r // 2], dm[2 + r % 2])), (name, L, size, sub, r)
                # pairwise
                out5 = g.alloc(5 * size * L * N)
                g.bfv_add_plain(L, size, 5, dc, dp, be.Context.pairwise(0, 1), out5, sub=sub)
                got = out5.download((5, size, L, N))
                for r in range(5):
                    assert np.array_equal(got[r], op(cts[r], dm[1 + r])), (name, L, size, sub, r)
                # in place: pairwise, and one plaintext for every ciphertext (b1 == 1)
                w = g.to_device(cts)
                g.bfv_add_plain(L, size, 5, w, dp, be.Context.pairwise(0, 0), w, sub=sub)
                got = w.download((5, size, L, N))
                for r in range(5):
                    assert np.array_equal(got[r], op(cts[r], dm[r])), (name, L, size, sub, r)
                w.upload(cts)
                g.bfv_add_plain(L, size, 5, w, dp, be.Context.outer(0, 5, 4, 1), w, sub=sub)
                got = w.download((5, size, L, N))
                for r in range(5):
                    assert np.array_equal(got[r], op(cts[r], dm[4])), (name, L, size, sub, r)
                # refused: in place when a ciphertext serves two results, and any partial overlap
                w.upload(cts)
                refused(be, lambda: g.bfv_add_plain(L, size, 4, w, dp, be.Context.outer(0, 2, 0, 2), w, sub=sub))
                refused(be, lambda: g.bfv_add_plain(L, size, 3, w, dp, be.Context.pairwise(1, 0), w, sub=sub))
                assert np.array_equal(w.download((5, size, L, N)), cts)
                for b in (out, out5, w):
                    b.free()
    refused(be, lambda: g.bfv_add_plain(g.L + 1, 2, 1, dc, dp, be.Context.pairwise(), dc))
    refused(be, lambda: g.bfv_add_plain(g.L, 4, 1, dc, dp, be.Context.pairwise(), dc))
    g.close()


@pytest.mark.parametrize("name", list(ALL))
def test_multiply_plain(be, oracle, name):
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(13)
    g.set_dual_stream(True)
    for L in range(1, g.L + 1):
        for size in (2, 3):
            cts, pls = rand_cts(o, rng, 8, L, size), plains(o, rng, 8, N)
            dc, dp = g.to_device(cts), g.to_device(pls)
            # outer product 3 x 2 (ciphertexts 1..3, plaintexts 0..1: the monomial and zero), then pairwise 8 (monomial, zero, -X^(N-1), full range)
            for n, ix, ia, ib in ((6, be.Context.outer(1, 3, 0, 2), lambda r: 1 + r // 2, lambda r: r % 2),
                                  (8, be.Context.pairwise(0, 0), lambda r: r, lambda r: r)):
                want = [mul_plain_transform(o, cts[ia(r)], pls[ib(r)]) for r in range(n)]
                out = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
                g.set_chunk(1024)
                g.bfv_multiply_plain(L, size, n, dc, dp, ix, out)
                got = out.download((n, size, L, N))
                for r in range(n):
                    assert np.array_equal(got[r], want[r]), (name, L, size, n, r)
                # the batch cut in chunks of 3, alternating over the two streams: same bits
                out3 = g.to_device(np.full(n * size * L * N, SENT, dtype=np.uint64))
                g.set_chunk(3)
                g.bfv_multiply_plain(L, size, n, dc, dp, ix, out3)
                assert np.array_equal(out3.download((n, size, L, N)), got), (name, L, size, n)
                g.set_chunk(1024)
                if N == 1024:  # (ii) no transform at all: schoolbook negacyclic convolution, 64 coefficients of every polynomial
                    js = [0, 1, 2, N - 1, N - 2, N // 2] + [int(v) for v in rng.choice(np.arange(3, N - 2), 58, replace=False)]
                    for r in (0, n - 1, 2):
                        lm = lift(o, pls[ib(r)], L)
                        for k in range(size):
                            for i in range(L):
                                assert [int(got[r, k, i, j]) for j in js] == schoolbook(cts[ia(r), k, i], lm[i], o.moduli[i], js), (L, size, r, k, i)
                # a zero plaintext gives a zero ciphertext; the monomial X^5 is a negacyclic shift
                rz = 1
                assert not got[rz].any()
                x5 = np.empty_like(cts[ia(0)])
                for i, q in enumerate(o.moduli[:L]):
                    c = cts[ia(0)][:, i]
                    x5[:, i, 5:] = c[:, :N - 5]
                    x5[:, i, :5] = (np.uint64(q) - c[:, N - 5:]) % np.uint64(q)
                assert np.array_equal(got[0], x5)
                out.free()
                out3.free()
            # refusals: any overlap of the output with an input; the output stays as it was
            w = g.to_device(cts)
            refused(be, lambda: g.bfv_multiply_plain(L, size, 8, w, dp, be.Context.pairwise(), w))
            refused(be, lambda: g.bfv_multiply_plain(L, size, 1, dc, w, be.Context.pairwise(), w))
            assert np.array_equal(w.download((8, size, L, N)), cts)
            for b in (dc, dp, w):
                b.free()
    g.close()


@pytest.mark.parametrize("name", ["n8192_default", "n1024", "n32768_d3"])
def test_async_producer_then_each_op(be, oracle, name):
    """The operand is still being written by he355_add (asynchronous, first stream) when each op is issued; the batch is cut in chunks of 3
    that alternate over both streams, so the second stream has to be ordered behind the producer."""
    g, o, N, *_ = pair(be, oracle, name)
    rng = np.random.default_rng(14)
    L, size, n = g.L, 2, 8
    g.set_dual_stream(True)
    g.set_chunk(3)
    x, y, pls = rand_cts(o, rng, n, L), rand_cts(o, rng, n, L), plains(o, rng, n, N)
    a_host = np.stack([o.add(x[r], y[r]) for r in range(n)])
    dx, dy, dp = g.to_device(x), g.to_device(y), g.to_device(pls)
    zeros = np.zeros((1, L, N), dtype=np.uint64)
    for rep in range(3):
        a = g.to_device(np.zeros_like(x))
        o_ms, o_ap, o_sp, o_mp = g.alloc(n * 2 * N), g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
        g.sync()
        g.add(L, 2, n, dx, dy, be.Context.pairwise(), a)
        g.bfv_multiply_plain(L, size, n, a, dp, be.Context.pairwise(), o_mp)
        g.add(L, 2, n, dx, dy, be.Context.pairwise(), a)
        g.bfv_mod_switch(L, 1, size, n, a, o_ms)
        g.add(L, 2, n, dx, dy, be.Context.pairwise(), a)
        g.bfv_add_plain(L, size, n, a, dp, be.Context.pairwise(), o_ap)
        g.add(L, 2, n, dx, dy, be.Context.pairwise(), a)
        g.bfv_add_plain(L, size, n, a, dp, be.Context.pairwise(), o_sp, sub=True)
        mp, ms, ap, sp = o_mp.download((n, 2, L, N)), o_ms.download((n, 2, 1, N)), o_ap.download((n, 2, L, N)), o_sp.download((n, 2, L, N))
        for r in range(n):
            d = np.concatenate([delta(o, pls[r], L)[None], zeros])
            assert np.array_equal(ms[r], switch_to(o, a_host[r], 1)), (rep, r)
            assert np.array_equal(ap[r], addsub(o, a_host[r], d, False)) and np.array_equal(sp[r], addsub(o, a_host[r], d, True)), (rep, r)
            if rep == 0 or r in (0, 3, 7):
                assert np.array_equal(mp[r], mul_plain_transform(o, a_host[r], pls[r])), (rep, r)
            else:
                assert np.array_equal(mp[r], first_mp[r]), (rep, r)
        first_mp = mp
        for b in (a, o_ms, o_ap, o_sp, o_mp):
            b.free()
    g.close()


@pytest.mark.parametrize("N,bits", [(4096, [60, 40, 40, 60]), (8192, [60, 40, 60]), (1024, [50, 40, 50])])
def test_semantic_multiply_add_switch_decrypt(be, oracle, N, bits):
    """Dec(mod_switch_to(L')(Enc(x) (.) p + r)) = x p + r mod t slot-wise for every L' down to 1: real keys from the oracle, x, p, r uniform
    over the full centred range, evaluated on the GPU, decrypted by the oracle and by he355_decrypt + he355_bfv_decode at L'."""
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    assert g.moduli == o.moduli and g.t == o.t
    t, L = o.t, g.L
    codec = oracle.BatchCodec(N, t)
    rng = np.random.default_rng(N)
    sk = o.keygen_secret(21)
    pk = o.keygen_public(sk, 22)
    g.set_public_key(pk)
    g.set_secret_key(sk)
    n = 3
    x, p, r = (rng.integers(-(t // 2), t // 2 + 1, (n, N)) for _ in range(3))
    want = (x.astype(object) * p.astype(object) + r.astype(object)) % t
    want = np.where(want > t // 2, want - t, want).astype(np.int64)
    enc = lambda v: np.stack([codec.encode(row) for row in v])
    ct, prod, full = g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
    g.encrypt(n, g.to_device(enc(x)), 31, 0, ct)
    g.bfv_multiply_plain(L, 2, n, ct, g.to_device(enc(p)), be.Context.pairwise(), prod)
    g.bfv_add_plain(L, 2, n, prod, g.to_device(enc(r)), be.Context.pairwise(), full)
    for L_to in range(L, 0, -1):
        low = g.alloc(n * 2 * L_to * N)
        g.bfv_mod_switch(L, L_to, 2, n, full, low)
        cts = low.download((n, 2, L_to, N))
        dec, vals = g.alloc(n * N), g.alloc(n * N)
        g.decrypt(L_to, 2, n, low, dec)
        g.bfv_decode(n, dec, vals)
        got_dev = vals.download().view(np.int64).reshape(n, N)
        for k in range(n):
            v = codec.decode(o.bfv_decode_phase(o.decrypt_phase(cts[k], sk)))
            v = np.where(v > t // 2, v - t, v)
            assert np.array_equal(v, want[k]), (L_to, k, "oracle decryption")
            assert np.array_equal(got_dev[k], want[k]), (L_to, k, "device decryption")
    g.close()


def test_second_call_makes_no_raw_allocation(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n8192_default")
    rng = np.random.default_rng(15)
    L, n = g.L, 8
    g.set_chunk(3)
    dc, dp = g.to_device(rand_cts(o, rng, n, L)), g.to_device(plains(o, rng, n, N))
    out, low = g.alloc(n * 2 * L * N), g.alloc(n * 2 * N)
    stats = []
    for _ in range(3):
        g.bfv_mod_switch(L, 1, 2, n, dc, low)
        g.bfv_add_plain(L, 2, n, dc, dp, be.Context.pairwise(), out)
        g.bfv_add_plain(L, 2, n, dc, dp, be.Context.pairwise(), out, sub=True)
        g.bfv_multiply_plain(L, 2, n, dc, dp, be.Context.pairwise(), out)
        g.sync()
        stats.append(g.alloc_stats())
    assert stats[0]["raw_mallocs"] == stats[1]["raw_mallocs"] == stats[2]["raw_mallocs"], stats
    assert stats[0]["raw_frees"] == stats[1]["raw_frees"] == stats[2]["raw_frees"], stats
    g.close()
