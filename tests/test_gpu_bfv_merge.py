"""GPU parity of the BFV ciphertext merge (he355_bfv_merge), bit-exact (np.array_equal, no tolerance):

* definition : every result against the definition run in the oracle (bfv_merge_ref.merge_levels: oracle.add / oracle.sub / oracle.apply_galois
               and a numpy shift), n1024 at L = 2 (Shoup form), n4096_d3 at L = 3 and L = 2 (fold form), count in {1, 2, 3, 5, 8, 16}, n in
               {1, 3}, the inputs child-major (n, 1), row-major (1, count) and padded (n + 1, 1) with sentinels in the gaps; result 0 merges
               real encryptions, the others random_poly ciphertexts with all-0 and all-(q - 1) rows; keys from oracle.keygen_galois; a sentinel
               before and after the output, the inputs read back; again under set_chunk(2); again behind an unsynchronised he355_add;
* composition: the same results bit for bit against the loop of the public device calls (bfv_multiply_monomial, add, sub, apply_galois, add);
* deep tree  : (2048, {60, 40, 60}), count = 2048, n = 1 (11 levels, shifts up to a whole 1024-word row), real keys, full-range plaintexts:
               decrypted on the device the result equals the closed form, and it equals the oracle's bit for bit;
* round trip : n4096_d3, expand -> merge at count 16 decrypts to 256 m;
* end to end : n4096_d3, four queries 2^-2 X^idx -> expand -> to_ntt -> multiply_plain_accumulate over a 4 x 2 database whose records sit on
               the coefficients that are multiples of 4 -> from_ntt -> bfv_merge(count = 4) -> he355_bfv_mod_switch to L = 1 -> decrypt: 4 times
               the four records interleaved (the client multiplies by 4^-1 mod t), two reply ciphertexts instead of eight; the noise budget
               stays positive;
* refusals   : CKKS context, bad L, count 0 / N + 1, colliding and zero strides, a stride that wraps, a missing Galois key (named in the
               message; missing at the second level, nothing is written), d_out over the inputs: the code, a message, the output untouched;
* a second identical he355_bfv_merge makes no raw hipMalloc."""

import numpy as np
import pytest

from bfv_gpu_helpers import SENT, At, be, edged, expand_keys, keyed, pair, rand_cts, refused, to_level  # noqa: F401 (be: the fixture)
from bfv_merge_ref import merge_levels, merged_plain

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
COUNTS = (1, 2, 3, 5, 8, 16)
KMAX, NMAX = 16, 3


_CASES = {}


def merge_case(be, oracle, chain, L):
    """a device / oracle pair with the Galois keys of a depth-4 tree, the inputs x [16][3][2][L][N] (input k of result r: result 0 real
    encryptions, results 1 and 2 edged random_poly ciphertexts) and want[count][r], the oracle's merge of x[:count, r] -- made once, shared
    by the tests below and left unchanged"""
    if (chain, L) not in _CASES:
        g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
        rng = np.random.default_rng(73 + L)
        gks = expand_keys(g, o, sk, KMAX, 180)
        x = np.empty((KMAX, NMAX, 2, L, N), dtype=np.uint64)
        for k in range(KMAX):
            x[k, 0] = to_level(o, o.encrypt(pk, rng.integers(0, o.t, N, dtype=np.uint64), 190 + k), L)
        x[:, 1] = edged(o, rng, KMAX, L)
        x[:, 2] = edged(o, rng, KMAX, L)[::-1]
        want = {c: [merge_levels(o, list(x[:c, r]), c, gks, L) for r in range(NMAX)] for c in COUNTS}
        _CASES[(chain, L)] = (g, o, N, x, want)
    return _CASES[(chain, L)]


def laid_out(x, count, n, layout):
    """(host slab [slots][2][L][N], stride_k, stride_r) of inputs x[:count, :n]; `padded` leaves a sentinel ciphertext behind every n"""
    if layout == "child":
        return np.ascontiguousarray(x[:count, :n]).reshape((count * n,) + x.shape[2:]), n, 1
    if layout == "row":
        return np.ascontiguousarray(x[:count, :n].swapaxes(0, 1)).reshape((count * n,) + x.shape[2:]), 1, count
    h = np.full((count, n + 1) + x.shape[2:], SENT, dtype=np.uint64)
    h[:, :n] = x[:count, :n]
    return h.reshape((count * (n + 1),) + x.shape[2:]), n + 1, 1


def check_results(got, want, count, n, what):
    for r in range(n):
        assert np.array_equal(got[r], want[count][r]), (what, "count", count, "n", n, "result", r)


MERGE_CASES = [("n1024", 2), ("n4096_d3", 3), ("n4096_d3", 2)]


@pytest.mark.parametrize("chain,L", MERGE_CASES)
def test_merge_equals_the_definition(be, oracle, chain, L):
    g, o, N, x, want = merge_case(be, oracle, chain, L)
    per = 2 * L * N
    for n in (1, NMAX):
        for count in COUNTS:
            for layout in ("child", "row", "padded"):
                h, sk_, sr_ = laid_out(x, count, n, layout)
                din = g.to_device(h)
                buf = g.to_device(np.full(n * per + 2 * N, SENT, dtype=np.uint64))
                g.bfv_merge(L, n, count, din, sk_, sr_, At(buf, N))
                got = buf.download()
                assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), (count, n, layout, "sentinel")
                check_results(got[N:-N].reshape(n, 2, L, N), want, count, n, layout)
                assert np.array_equal(din.download(h.shape), h), (count, n, layout, "inputs")
                din.free()
                buf.free()


@pytest.mark.parametrize("chain,L", MERGE_CASES)
def test_merge_in_ragged_chunks(be, oracle, chain, L):
    """set_chunk(2): the 12, 6, 3 (count 5) and 24, 12, 6, 3 (count 16) key switches of the level batches are cut into chunks of two"""
    g, o, N, x, want = merge_case(be, oracle, chain, L)
    n = NMAX
    g.set_chunk(2)
    try:
        for count, layout in ((5, "row"), (16, "child")):
            h, sk_, sr_ = laid_out(x, count, n, layout)
            din, out = g.to_device(h), g.alloc(n * 2 * L * N)
            g.bfv_merge(L, n, count, din, sk_, sr_, out)
            check_results(out.download((n, 2, L, N)), want, count, n, "chunk 2")
            din.free()
            out.free()
    finally:
        g.set_chunk(1024)


@pytest.mark.parametrize("chain,L", MERGE_CASES)
def test_merge_behind_an_unsynchronised_producer(be, oracle, chain, L):
    g, o, N, x, want = merge_case(be, oracle, chain, L)
    n, count = NMAX, 8
    h, sk_, sr_ = laid_out(x, count, n, "child")
    rng = np.random.default_rng(74)
    y = rand_cts(o, rng, count * n, L)
    a = np.stack([o.sub(h[i], y[i]) for i in range(count * n)])  # a + y = the inputs
    da, dy = g.to_device(a), g.to_device(y)
    din, out = g.to_device(np.zeros_like(h)), g.alloc(n * 2 * L * N)
    g.sync()
    g.add(L, 2, count * n, da, dy, be.Context.pairwise(), din)
    g.bfv_merge(L, n, count, din, sk_, sr_, out)
    check_results(out.download((n, 2, L, N)), want, count, n, "producer")
    for b in (da, dy, din, out):
        b.free()


def composed(be, g, L, N, n, count, din, out):
    """the definition from the public device calls, inputs child-major in `din`: per level bfv_multiply_monomial, add, sub, apply_galois, add"""
    per = 2 * L * N
    d = (count - 1).bit_length()
    pw = be.Context.pairwise()
    half = max(1, (1 << d) // 2) * n
    mono, S, D, G = (g.alloc(half * per) for _ in range(4))
    cur, have = din, count
    mids = []
    for j in range(d - 1, -1, -1):
        s, e = 1 << j, N // (1 << j) + 1
        full, rest = (have - s) * n, (2 * s - have) * n  # pairs with a partner, pairs without
        dst = out if j == 0 else g.alloc(s * n * per)
        g.bfv_multiply_monomial(L, 2, full, At(cur, s * n * per), s, mono)
        g.add(L, 2, full, cur, mono, pw, S)
        g.add(L, 2, full, cur, mono, pw, D, sub=True)
        g.apply_galois(L, full, D, e, G)
        g.add(L, 2, full, S, G, pw, dst)
        if rest:  # S = D = even
            g.apply_galois(L, rest, At(cur, full * per), e, At(G, full * per))
            g.add(L, 2, rest, At(cur, full * per), At(G, full * per), pw, At(dst, full * per))
        if j:
            mids.append(dst)
        cur, have = dst, s
    g.sync()
    for b in [mono, S, D, G] + mids:
        b.free()


@pytest.mark.parametrize("chain,L,count", [("n1024", 2, 5), ("n4096_d3", 3, 16), ("n4096_d3", 2, 3)])
def test_merge_equals_the_composition_of_the_public_calls(be, oracle, chain, L, count):
    g, o, N, x, want = merge_case(be, oracle, chain, L)
    n = NMAX
    h, sk_, sr_ = laid_out(x, count, n, "child")
    din, a, b = g.to_device(h), g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
    g.bfv_merge(L, n, count, din, sk_, sr_, a)
    composed(be, g, L, N, n, count, din, b)
    got, ref = a.download((n, 2, L, N)), b.download((n, 2, L, N))
    assert np.array_equal(got, ref)
    check_results(got, want, count, n, "composition")
    for buf in (din, a, b):
        buf.free()


def test_second_identical_merge_makes_no_raw_allocation(be, oracle):
    g, o, N, x, want = merge_case(be, oracle, "n4096_d3", 3)
    n, count, L = NMAX, 16, 3
    h, sk_, sr_ = laid_out(x, count, n, "child")
    din, out = g.to_device(h), g.alloc(n * 2 * L * N)
    g.bfv_merge(L, n, count, din, sk_, sr_, out)
    g.sync()
    first = g.alloc_stats()
    g.bfv_merge(L, n, count, din, sk_, sr_, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    check_results(out.download((n, 2, L, N)), want, count, n, "second call")
    din.free()
    out.free()


# ---- what the result decrypts to --------------------------------------------------------------------------------------------------
def test_deep_tree(be, oracle):
    """count = N = 2048: 11 levels, 2047 key switches, the first level's shift a whole 1024-word row"""
    count = 2048
    g, o, N, sk, pk, gks = keyed(be, oracle, N2048, count, 200)
    assert N == count and len(gks) == 11 and min(gks) == 3
    L, t = g.L, o.t
    rng = np.random.default_rng(75)
    mu = rng.integers(0, t, (count, N), dtype=np.uint64)
    mu[0, 0], mu[1, 0], mu[2, 0], mu[3, 0] = 0, 1, t - 1, t // 2
    cts = np.stack([o.encrypt(pk, mu[k], 500 + k) for k in range(count)])
    din, out, dec = g.to_device(cts), g.alloc(2 * L * N), g.alloc(N)
    g.bfv_merge(L, 1, count, din, 1, 1, out)
    g.decrypt(L, 2, 1, out, dec)
    assert np.array_equal(dec.download((N,)), merged_plain(mu, t))
    budget = g.bfv_noise_budget(L, 2, 1, out)
    print(f"deep tree: noise budget of the merged ciphertext {budget.min()} bits")
    assert (budget > 0).all()
    assert np.array_equal(out.download((2, L, N)), merge_levels(o, list(cts), count, gks, L))
    g.close()


def test_round_trip_and_end_to_end(be, oracle):
    g, o, N, sk, pk, gks = keyed(be, oracle, "n4096_d3", 16, 240)
    L, t = g.L, o.t
    assert L == 3
    per = 2 * L * N
    rng = np.random.default_rng(76)
    # expand -> merge at count 16: 4^4 m
    m = rng.integers(0, t, (1, N), dtype=np.uint64)
    query, kids, back, dec = g.alloc(per), g.alloc(16 * per), g.alloc(per), g.alloc(N)
    g.encrypt(1, g.to_device(m), 94, 0, query)
    g.bfv_expand(L, 1, query, 16, kids)
    g.bfv_merge(L, 1, 16, kids, 1, 1, back)
    g.decrypt(L, 2, 1, back, dec)
    assert np.array_equal(dec.download((N,)), (m[0].astype(object) * 256 % t).astype(np.uint64))
    assert (g.bfv_noise_budget(L, 2, 1, back) > 0).all()
    # four retrievals, one reply ciphertext per column instead of four
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
    g.bfv_multiply_plain_accumulate(L, 2, nq, cols, rows, kids4, 1, nq, ptn, cols, 1, res)  # result (query r, column j) at r cols + j
    g.bfv_transform_from_ntt(L, 2, nq * cols, res, res)
    scanned = g.bfv_noise_budget(L, 2, nq * cols, res)
    g.bfv_merge(L, cols, nq, res, cols, 1, reply)  # input k = query k, result r = column r
    merged = g.bfv_noise_budget(L, 2, cols, reply)
    cur = reply
    for Lc in (2, 1):
        nxt = g.alloc(cols * 2 * Lc * N)
        g.bfv_mod_switch(Lc + 1, Lc, 2, cols, cur, nxt)
        cur = nxt
    final = g.bfv_noise_budget(1, 2, cols, cur)
    out = g.alloc(cols * N)
    g.decrypt(1, 2, cols, cur, out)
    got = out.download((cols, N))
    want = np.zeros((cols, N), dtype=np.uint64)
    for j in range(cols):
        for k in range(nq):  # coefficient k + 4 m carries record idx[k]'s coefficient 4 m, times 4
            want[j, k::4] = (db[idx[k], j, ::4].astype(object) * 4 % t).astype(np.uint64)
    assert np.array_equal(got, want)
    inv4 = pow(4, -1, t)
    client = (got.astype(object) * inv4 % t).astype(np.uint64)  # what the client reads: the four records interleaved
    for j in range(cols):
        for k in range(nq):
            assert np.array_equal(client[j, k::4], db[idx[k], j, ::4])
    print(f"end to end: noise budgets (bits) scanned {scanned.min()}..{scanned.max()}, merged {merged.min()}..{merged.max()}, at L = 1 {final.min()}..{final.max()};"
          f" reply {cols * 2 * N * 8} bytes instead of {nq * cols * 2 * N * 8}")
    for v in (scanned, merged, final):
        assert (v > 0).all(), v
    g.close()


def test_refusals(be, oracle):
    g, o, N, sk, _ = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(77)
    L = g.L
    per = 2 * L * N
    x = rand_cts(o, rng, 8, L)
    dx = g.to_device(x)
    out = g.to_device(np.full(12 * per, SENT, dtype=np.uint64))
    merge = lambda L_=L, n=2, count=4, src=dx, sk_=2, sr_=1, dst=out: g.bfv_merge(L_, n, count, src, sk_, sr_, dst)
    elts = g.bfv_expand_galois_elts(4)
    assert elts == [N + 1, N // 2 + 1]
    with pytest.raises(be.HE355Error) as ei:  # no Galois key at all: the first level's (j = 1) is named
        merge()
    assert ei.value.code == be.E_INVALID_ARGS and str(N // 2 + 1) in str(ei.value)
    g.set_galois_key(elts[1], o.keygen_galois(sk, elts[1], 71))
    with pytest.raises(be.HE355Error) as ei:  # the second level's key is missing: nothing of the first level may have run
        merge()
    assert ei.value.code == be.E_INVALID_ARGS and str(N + 1) in str(ei.value)
    assert (out.download() == SENT).all()
    g.set_galois_key(elts[0], o.keygen_galois(sk, elts[0], 70))
    refused(be, lambda: merge(count=0))
    refused(be, lambda: merge(count=N + 1))
    refused(be, lambda: merge(L_=0))
    refused(be, lambda: merge(L_=L + 1))
    refused(be, lambda: merge(sk_=0))
    refused(be, lambda: merge(sr_=0))
    refused(be, lambda: merge(sk_=1, sr_=1))
    refused(be, lambda: merge(count=3, sk_=2, sr_=4))
    refused(be, lambda: merge(sk_=1 << 63))
    refused(be, lambda: merge(sr_=1 << 50, sk_=1))
    refused(be, lambda: merge(src=out))
    refused(be, lambda: merge(src=At(out, per)))                # the output's second ciphertext is the first input
    refused(be, lambda: merge(src=At(out, N), count=1, n=1))    # count == 1 is a copy: it may not run over itself either
    refused(be, lambda: merge(src=out, count=2, sk_=3, dst=At(out, 2 * per), n=2))  # inside a gap of padded inputs
    merge(n=0)
    assert (out.download() == SENT).all()
    assert np.array_equal(dx.download((8, 2, L, N)), x)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(8 * per), ck.to_device(np.full(2 * per, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_merge(ck.L, 2, 4, a, 2, 1, b))
    assert (b.download() == SENT).all()
    ck.close()
