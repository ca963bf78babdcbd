"""GPU parity of BFV reply compression (he355_bfv_reply_compress, he355_bfv_reply_decrypt), bit-exact (np.array_equal, no tolerance) against
the definition in Python integers (tests/bfv_reply_ref.py, held to itself in test_bfv_reply_ref_cpu.py):

* compress   : n1024 (Shoup form) and n4096_d3 (fold form); three `edged` ciphertexts (all-0, all-(q - 1) and alternating rows) plus two
               uniform ones; widths (22, 32), the safe pair, (2, 2), (31, 33) and k0 = k1 = the chain's largest accepted width; at L = 1, and
               at L = L_top against to_level (the oracle's mod_switch_to_next chain) followed by the reference; every reply lands at a
               stride of the reply size + 24 bytes inside a sentinelled buffer: the gaps and both guards are intact; the operands are
               read back unchanged;
* decrypt    : the same widths on uniformly random reply bytes (the definition is total: no valid ciphertext is needed), and on replies of
               all ones and all zeros; under the oracle's key and the constant keys +1 and -1; n = 65 at N = 1024, which crosses the
               64-reply chunk, and once more after set_chunk(2); plaintext, budget and noise_bits; NULL and non-NULL budget outputs give the
               same plaintext; the product's reference is the oracle's transform pair around a product in Python integers;
* large ring : n32768_d3, n = 2, safe widths: compress at L = 3; decrypt against the reference, whose product is checked on 64 sampled
               coefficients against the integer sum over the key's coefficients;
* end to end : the merge module's retrieval (N = 4096 {60, 40, 40, 60}, records on every fourth coefficient): the replies taken to L = 1 have
               a noise budget of at least 2 bits; compressed with the safe widths, downloaded, uploaded on a second context that holds only
               the secret key and decrypted there, they equal he355_decrypt of the uncompressed replies and the database records; a reply is
               bfv_reply_bytes long, less than 2 N 8;
* refusals   : with a device behind the context, the missing secret key included: the code, a message, the outputs untouched."""
import numpy as np
import pytest

import bfv_reply_ref as ref
from bfv_gpu_helpers import SENT, At, be, edged, expand_keys, inner_of, keyed, pair, rand_cts, refused, sentinelled, to_level  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

CHAINS = ("n1024", "n4096_d3")
PAD = 24  # bytes between two replies


def widths_of(g, N):
    q = int(g.moduli[0])
    k0, k1, ok = g.bfv_reply_safe_bits()
    assert ok and (k0, k1) == ref.safe_bits(N, g.t)
    top = ref.max_width(N, q)
    out = []
    for w in ((22, 32), (k0, k1), (2, 2), (31, 33), (top, top)):
        if w not in out:
            out.append(w)
    assert all(ref.accepted(N, q, *w) for w in out) and not ref.accepted(N, q, 2, top + 1)
    return out


def as_words(data, stride):
    """[n][B] uint8 -> the uint64 words of n replies `stride` bytes apart, the gaps filled with the sentinel"""
    n, B = data.shape
    h = np.full((n, stride // 8), SENT, dtype=np.uint64)
    h.view(np.uint8).reshape(n, stride)[:, :B] = data
    return h.reshape(-1)


_OPERANDS = {}


def operands(be, oracle, chain):
    """(g, o, N, x, low): five ciphertexts at L_top (three edged, two uniform), and the same at L = 1 by the oracle -- made once, left unchanged"""
    if chain not in _OPERANDS:
        g, o, N, _, _ = pair(be, oracle, chain)
        rng = np.random.default_rng(310 + N)
        x = np.concatenate((edged(o, rng, 3, g.L), rand_cts(o, rng, 2, g.L)))
        low = np.stack([to_level(o, c, 1) for c in x])
        _OPERANDS[chain] = (g, o, N, x, low)
    return _OPERANDS[chain]


def check_compress(g, N, L, ct, want_low, q, k0, k1):
    n = ct.shape[0]
    B = g.bfv_reply_bytes(k0, k1)
    assert B == ref.reply_bytes(N, k0, k1)
    stride = B + PAD
    din = g.to_device(ct)
    buf = sentinelled(g, n * stride // 8, N)
    g.bfv_reply_compress(L, k0, k1, n, din, buf, stride, byte_offset=8 * N)
    got = inner_of(buf, N, (L, k0, k1)).view(np.uint8).reshape(n, stride)
    want = ref.np_compress(want_low, q, k0, k1)
    assert np.array_equal(got[:, :B], want), (L, k0, k1)
    assert (got[:, B:].reshape(-1).view(np.uint64) == SENT).all(), (L, k0, k1, "gaps")
    assert np.array_equal(din.download(ct.shape), ct), (L, k0, k1, "operands")
    din.free()
    buf.free()


@pytest.mark.parametrize("chain", CHAINS)
def test_compress_equals_the_reference(be, oracle, chain):
    g, o, N, x, low = operands(be, oracle, chain)
    q = int(g.moduli[0])
    rng = np.random.default_rng(311)
    at1 = np.concatenate((edged(o, rng, 3, 1), rand_cts(o, rng, 2, 1)))
    for k0, k1 in widths_of(g, N):
        check_compress(g, N, 1, at1, at1, q, k0, k1)
        check_compress(g, N, g.L, x, low, q, k0, k1)


def product_ref(o, lifted, sk0, q):
    """[n][N] residues mod q_0 -> the residues of their negacyclic products with the key whose NTT form at prime 0 is sk0"""
    s = sk0.astype(object)
    return np.stack([o.intt(0, (o.ntt(0, row).astype(object) * s % q).astype(np.uint64)) for row in lifted])


def decrypt_ref(o, data, N, k0, k1, q, t, sk0):
    y0, y1 = ref.np_unpack(data, N, k0, k1)
    return ref.np_finish(y0, product_ref(o, ref.np_lift(y1, k1, q), sk0, q), k0, k1, q, t)


def run_decrypt(g, data, N, k0, k1, with_budget=True):
    n, B = data.shape
    stride = B + PAD
    dby = g.to_device(as_words(data, stride))
    out = sentinelled(g, n * N, N)
    res = g.bfv_reply_decrypt(k0, k1, n, dby, stride, At(out, N), with_budget=with_budget)
    plain = inner_of(out, N, (k0, k1)).reshape(n, N)
    assert np.array_equal(dby.download(), as_words(data, stride)), "the replies are read, not written"
    dby.free()
    out.free()
    return plain, res


def reply_bytes_for(rng, n, B):
    data = rng.integers(0, 256, (n, B), dtype=np.uint8)
    data[n - 2] = 0xFF
    data[n - 1] = 0
    return data


def keys_of(g, o):
    ones = np.ones((g.K, g.N), dtype=np.uint64)
    minus = np.stack([np.full(g.N, int(q) - 1, dtype=np.uint64) for q in g.moduli])
    return {"oracle": o.keygen_secret(21), "+1": ones, "-1": minus}


@pytest.mark.parametrize("key", ["oracle", "+1", "-1"])
@pytest.mark.parametrize("chain", CHAINS)
def test_decrypt_equals_the_reference(be, oracle, chain, key):
    g, o, N, _, _ = operands(be, oracle, chain)
    q, t = int(g.moduli[0]), g.t
    sk = keys_of(g, o)[key]
    g.set_secret_key(sk)
    n = 65 if N == 1024 else 5
    rng = np.random.default_rng(320 + N)
    for k0, k1 in widths_of(g, N):
        data = reply_bytes_for(rng, n, g.bfv_reply_bytes(k0, k1))
        want, budget, bits = decrypt_ref(o, data, N, k0, k1, q, t, sk[0])
        plain, (gb, gn) = run_decrypt(g, data, N, k0, k1)
        assert np.array_equal(plain, want), (key, k0, k1)
        assert np.array_equal(gb, budget) and np.array_equal(gn, bits), (key, k0, k1, gb, budget, gn, bits)
        if key != "oracle":  # the product is -+ the centred c1 itself
            y0, y1 = ref.np_unpack(data[:1], N, k0, k1)
            sign = 1 if key == "+1" else -1
            w = [sign * ref.centre(int(v), k1) for v in y1[0]]
            assert [int(v) for v in want[0]] == ref.finish([int(v) for v in y0[0]], w, k0, k1, t)[0]


@pytest.mark.parametrize("chain", CHAINS)
def test_decrypt_in_small_chunks_and_without_budget_outputs(be, oracle, chain):
    g, o, N, _, _ = operands(be, oracle, chain)
    q, t = int(g.moduli[0]), g.t
    sk = o.keygen_secret(21)
    g.set_secret_key(sk)
    n = 65 if N == 1024 else 5
    k0, k1, _ = g.bfv_reply_safe_bits()
    data = reply_bytes_for(np.random.default_rng(330 + N), n, g.bfv_reply_bytes(k0, k1))
    want, budget, bits = decrypt_ref(o, data, N, k0, k1, q, t, sk[0])
    bare, none = run_decrypt(g, data, N, k0, k1, with_budget=False)
    assert none is None and np.array_equal(bare, want)
    # noise_bits alone, budget alone
    stride = data.shape[1] + PAD
    dby, out = g.to_device(as_words(data, stride)), g.alloc(n * N)
    stat = g.to_device(np.full(n, SENT, dtype=np.uint64))
    lib = be.lib()
    assert lib.he355_bfv_reply_decrypt(g.h, k0, k1, n, dby.ptr, stride, out.ptr, None, stat.ptr) == 0
    assert np.array_equal(stat.download().view(np.int32)[:n], bits) and (stat.download()[(n + 1) // 2:] == SENT).all()
    assert lib.he355_bfv_reply_decrypt(g.h, k0, k1, n, dby.ptr, stride, out.ptr, stat.ptr, None) == 0
    assert np.array_equal(stat.download().view(np.int32)[:n], budget) and np.array_equal(out.download((n, N)), want)
    g.set_chunk(2)
    try:
        plain, (gb, gn) = run_decrypt(g, data, N, k0, k1)
    finally:
        g.set_chunk(1024)
    assert np.array_equal(plain, want) and np.array_equal(gb, budget) and np.array_equal(gn, bits)
    for b in (dby, out, stat):
        b.free()


def test_one_large_ring(be, oracle):
    g, o, N, _, _ = pair(be, oracle, "n32768_d3")
    sk = o.keygen_secret(21)
    g.set_secret_key(sk)
    L, q, t, n = g.L, int(g.moduli[0]), g.t, 2
    assert L == 3
    k0, k1, ok = g.bfv_reply_safe_bits()
    assert ok and (k0, k1) == (22, 37) and g.bfv_reply_bytes(k0, k1) == 241664
    rng = np.random.default_rng(340)
    x = rand_cts(o, rng, n, L)
    low = np.stack([to_level(o, c, 1) for c in x])
    check_compress(g, N, L, x, low, q, k0, k1)
    data = ref.np_compress(low, q, k0, k1)
    y0, y1 = ref.np_unpack(data, N, k0, k1)
    prod = product_ref(o, ref.np_lift(y1, k1, q), sk[0], q)
    # the product on 64 sampled coefficients, from the key's coefficients: sum_i y1^[i] s[e - i], the wrapped terms negated (below 2^52)
    s = o.intt(0, sk[0]).astype(np.int64)
    s = np.where(s > q // 2, s - q, s)
    assert set(np.unique(s)) <= {-1, 0, 1}
    yc = y1.astype(np.int64)
    yc = np.where(yc >= 2 ** (k1 - 1), yc - 2 ** k1, yc)
    idx = np.arange(N)
    for j in range(n):
        for e in [0, 1, N - 1] + [int(v) for v in rng.integers(0, N, 61)]:
            terms = yc[j] * s[(e - idx) % N] * np.where(idx <= e, 1, -1)
            assert int(terms.sum()) % q == int(prod[j, e]), (j, e)
    want, budget, bits = ref.np_finish(y0, prod, k0, k1, q, t)
    plain, (gb, gn) = run_decrypt(g, data, N, k0, k1)
    assert np.array_equal(plain, want) and np.array_equal(gb, budget) and np.array_equal(gn, bits)
    g.close()


def test_end_to_end(be, oracle):
    g, o, N, sk, pk, gks = keyed(be, oracle, "n4096_d3", 4, 240)
    L, t = g.L, o.t
    per = 2 * L * N
    rng = np.random.default_rng(350)
    rows, nq, cols, idx = 4, 4, 2, (3, 0, 2, 2)
    db = np.zeros((rows, cols, N), dtype=np.uint64)
    db[:, :, ::4] = rng.integers(0, t, (rows, cols, N // 4), dtype=np.uint64)  # a record fills a quarter of the ring
    qp = np.zeros((nq, N), dtype=np.uint64)
    for r in range(nq):
        qp[r, idx[r]] = pow(4, -1, t)
    queries, kids4, ptn, res, reply = g.alloc(nq * per), g.alloc(rows * nq * per), g.alloc(rows * cols * L * N), g.alloc(nq * cols * per), g.alloc(cols * per)
    g.encrypt(nq, g.to_device(qp), 95, 0, queries)
    g.bfv_expand(L, nq, queries, rows, kids4)
    g.bfv_transform_to_ntt(L, 2, rows * nq, kids4, kids4)
    g.bfv_plain_to_ntt(L, rows * cols, g.to_device(db.reshape(rows * cols, N)), ptn)
    g.bfv_multiply_plain_accumulate(L, 2, nq, cols, rows, kids4, 1, nq, ptn, cols, 1, res)
    g.bfv_transform_from_ntt(L, 2, nq * cols, res, res)
    g.bfv_merge(L, cols, nq, res, cols, 1, reply)
    # the replies at L = 1: at least the 2 bits the safe widths ask for
    low = g.alloc(cols * 2 * N)
    g.bfv_mod_switch(L, 1, 2, cols, reply, low)
    final = g.bfv_noise_budget(1, 2, cols, low)
    assert (final >= 2).all(), final
    plain = g.alloc(cols * N)
    g.decrypt(1, 2, cols, low, plain)
    uncompressed = plain.download((cols, N))
    k0, k1, ok = g.bfv_reply_safe_bits()
    B = g.bfv_reply_bytes(k0, k1)
    assert ok and B == N * (k0 + k1) // 8 and B < 2 * N * 8
    wire = g.alloc(cols * B // 8)
    g.bfv_reply_compress(L, k0, k1, cols, reply, wire, B)  # from L = 3: the switch is part of the call
    sent = wire.download()
    assert sent.nbytes == cols * B
    g.close()
    # the client: a context that holds the secret key and nothing else
    c = be.Context(be.SCHEME_BFV, N, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False, device=0)
    c.set_secret_key(sk)
    out = c.alloc(cols * N)
    budget, bits = c.bfv_reply_decrypt(k0, k1, cols, c.to_device(sent), B, out, with_budget=True)
    got = out.download((cols, N))
    assert np.array_equal(got, uncompressed)
    inv4 = pow(4, -1, t)
    client = (got.astype(object) * inv4 % t).astype(np.uint64)  # what the client reads: the four records interleaved
    for j in range(cols):
        for k in range(nq):
            assert np.array_equal(client[j, k::4], db[idx[k], j, ::4])
    print(f"end to end: budget at L = 1 {final.min()}..{final.max()} bits; compressed ({k0}, {k1}): budget {budget.min()}..{budget.max()}, noise_bits {bits.min()}..{bits.max()};"
          f" reply {B} bytes instead of {2 * N * 8}")
    c.close()


def test_refusals(be, oracle):
    g, o, N, _, _ = pair(be, oracle, "n4096_d3")
    L = g.L
    k0, k1, _ = g.bfv_reply_safe_bits()
    B = g.bfv_reply_bytes(k0, k1)
    rng = np.random.default_rng(360)
    x = rand_cts(o, rng, 2, L)
    dx = g.to_device(x)
    by = g.to_device(np.full(2 * (B + PAD) // 8 + 2 * N, SENT, dtype=np.uint64))
    pl = g.to_device(np.full(2 * N + 2, SENT, dtype=np.uint64))
    comp = lambda L_=L, a=k0, b=k1, n=2, src=dx, dst=by, stride=B, off=0: g.bfv_reply_compress(L_, a, b, n, src, dst, stride, byte_offset=off)
    lib = be.lib()

    def dec(a=k0, b=k1, n=2, src=by, stride=B, dst=pl, bud=None, bits=None):
        code = lib.he355_bfv_reply_decrypt(g.h, a, b, n, src.ptr, stride, dst.ptr, bud, bits)
        if code:
            raise be.HE355Error(code, lib.he355_last_error().decode())

    with pytest.raises(be.HE355Error) as ei:  # no secret key: named, before any launch
        dec()
    assert ei.value.code == be.E_INVALID_ARGS and "secret key" in str(ei.value) and "he355_bfv_reply_decrypt" in str(ei.value)
    assert (pl.download() == SENT).all()
    g.set_secret_key(o.keygen_secret(21))
    top = ref.max_width(N, int(g.moduli[0]))
    for f in (lambda: comp(L_=0), lambda: comp(L_=L + 1), lambda: comp(a=1), lambda: comp(a=k1 + 1), lambda: comp(a=2, b=top + 1),
              lambda: comp(off=4), lambda: comp(stride=B - 8), lambda: comp(stride=B + 4), lambda: comp(n=3, stride=1 << 62),
              lambda: comp(n=(2 ** 31 - 1) // (N // 256) + 1, a=2, b=2, stride=N // 2), lambda: comp(dst=dx), lambda: comp(src=by),
              lambda: dec(a=1), lambda: dec(a=2, b=top + 1), lambda: dec(stride=B - 8), lambda: dec(stride=B + 4), lambda: dec(dst=by),
              lambda: dec(bud=by.ptr), lambda: dec(bits=pl.ptr), lambda: dec(bud=C_at(pl, 8 * 2 * N), bits=C_at(pl, 8 * 2 * N + 4))):
        refused(be, f)
    comp(n=0)
    dec(n=0)
    assert (by.download() == SENT).all() and (pl.download() == SENT).all()
    assert np.array_equal(dx.download(x.shape), x)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(2 * 2 * ck.L * N), ck.to_device(np.full(2 * B // 8, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_reply_compress(ck.L, k0, k1, 2, a, b, B))
    refused(be, lambda: ck.bfv_reply_decrypt(k0, k1, 2, b, B, a))
    assert (b.download() == SENT).all()
    assert ck.bfv_reply_bytes(k0, k1) == 0
    ck.close()


def C_at(buf, byte_offset):
    import ctypes
    return ctypes.c_void_p(buf.ptr.value + byte_offset)
