"""GPU parity of the BFV ciphertext decomposition for recursive (two-dimensional) PIR (he355_bfv_digit_count, he355_bfv_decompose,
he355_bfv_decompose_ntt, he355_bfv_compose), bit-exact (np.array_equal, no tolerance):

* decompose / compose against numpy integers: chains n1024 (Shoup form, no column pass), (2048, {60, 40, 60}) (the smallest column pass) and
  n4096_d3 (fold form, both engines); L in {L_top, 1}; sizes 1..3; n in {1, 3}; uniform rows mixed with all-0, all-(q - 1) and alternating
  rows; a sentinel before and after the output, the input read back; compose(decompose(x)) == x; compose of full-range random words
  against the masked sum in numpy;
* he355_bfv_decompose_ntt == he355_bfv_decompose + he355_bfv_plain_to_ntt: the same chains, every (L, L_out) in {1, L_top}^2, sizes 2 and
  3, n in {1, 3}; again behind an unsynchronised he355_add.  (A block of the fused column pass owns a quarter of ONE polynomial's columns,
  so no count of polynomials leaves a block ragged; n = 3 with F odd or even covers odd totals all the same.)
* refusals  : CKKS context, bad L / L_out, size 0 / 4, every overlap: the code, a message, and the output untouched; n == 0 touches nothing;
* end to end: n4096_d3, real keys, an 8 x 8 database of full-range plaintexts, two queries Enc(2^-4 (X^i + X^(8 + j))): expand(16) -> to_ntt
  -> scan over children 0..7 (8 results per query) -> from_ntt -> mod_switch to L = 1 -> decompose_ntt (L = 1 -> L_out = 3) -> scan of
  children 8..15 against the F columns -> from_ntt -> decrypt (F plaintexts per query) -> compose at L = 1 -> decrypt at L = 1 gives
  database entry (i, j) exactly; the noise budget is positive after every stage (printed);
* a second identical he355_bfv_decompose_ntt makes no raw hipMalloc (the fused path, and N = 1024's pool block), and he355_bfv_route_stats says
  which of the two ran."""

import numpy as np
import pytest

from bfv_gpu_helpers import SENT, At, be, edged, expand_keys, inner_of, pair, rand_cts, refused, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
CHAINS = ["n1024", N2048, "n4096_d3"]
IDS = ["n1024", "n2048", "n4096_d3"]


def table(moduli, t):
    w = t.bit_length() - 1
    D = [-(-q.bit_length() // w) for q in moduli]
    return w, D, sum(D)


def np_digits(x, moduli, t):
    """[n][size][L][N] canonical residues -> [n][size * D(L)][N] digits, polynomial k, prime i, digit g at k D(L) + off_i + g"""
    n, size, L, N = x.shape
    w, D, total = table(moduli[:L], t)
    out = np.empty((n, size, total, N), dtype=np.uint64)
    mask = np.uint64((1 << w) - 1)
    for k in range(size):
        f = 0
        for i in range(L):
            for g in range(D[i]):
                out[:, k, f, :] = (x[:, k, i, :] >> np.uint64(g * w)) & mask
                f += 1
    return out.reshape(n, size * total, N)


def np_compose(d, moduli, t, size, L):
    """[n][F][N] arbitrary words -> [n][size][L][N]: the masked sum, reduced"""
    n, F, N = d.shape
    w, D, total = table(moduli[:L], t)
    d = d.reshape(n, size, total, N)
    out = np.empty((n, size, L, N), dtype=np.uint64)
    for k in range(size):
        f = 0
        for i in range(L):
            q, b = np.uint64(moduli[i]), moduli[i].bit_length()
            s = np.zeros((n, N), dtype=np.uint64)
            for g in range(D[i]):
                keep = w if g + 1 < D[i] else b - (D[i] - 1) * w
                s += (d[:, k, f, :] & np.uint64((1 << keep) - 1)) << np.uint64(g * w)
                f += 1
            out[:, k, i, :] = np.where(s >= q, s - q, s)
    return out


def test_np_reference_on_small_integers():
    q, t = [(1 << 60) - 93, (1 << 39) + 1], 1032193
    x = np.array([[[[0, 1, q[0] - 1, q[0] // 2]], [[5, (1 << 38) + 7, q[1] - 1, 1 << 19]]]], dtype=np.uint64).reshape(1, 1, 2, 4)
    d = np_digits(x, q, t)
    w, D, total = table(q, t)
    assert (w, D) == (19, [4, 3]) and d.shape == (1, 7, 4) and (d < 2 ** w).all()
    for i in range(2):
        for e in range(4):
            off = sum(D[:i])
            assert sum(int(d[0, off + g, e]) << (g * w) for g in range(D[i])) == int(x[0, 0, i, e])
    assert np.array_equal(np_compose(d, q, t, 1, 2), x)


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_decompose_and_compose(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(73)
    for L in sorted({g.L, 1}):
        total, D = g.bfv_digit_count(L)
        assert (D, total) == table(o.moduli[:L], o.t)[1:]
        for size in (1, 2, 3):
            F = size * total
            for n in (1, 3):
                what = (L, size, n)
                x = edged(o, rng, n, L, size)
                dx = g.to_device(x)
                buf = sentinelled(g, n * F * N, N)
                g.bfv_decompose(L, size, n, dx, At(buf, N))
                want = np_digits(x, o.moduli, o.t)
                assert np.array_equal(inner_of(buf, N, what).reshape(n, F, N), want), (what, "digits")
                assert np.array_equal(dx.download((n, size, L, N)), x), (what, "input")
                back = sentinelled(g, n * size * L * N, N)
                g.bfv_compose(L, size, n, At(buf, N), At(back, N))
                assert np.array_equal(inner_of(back, N, what).reshape(n, size, L, N), x), (what, "compose o decompose")
                assert np.array_equal(inner_of(buf, N, what).reshape(n, F, N), want), (what, "compose's input")
                words = rng.integers(0, 2 ** 64, (n, F, N), dtype=np.uint64)  # full-range "digits"
                words[0, 0, :] = 2 ** 64 - 1
                dw = g.to_device(words)
                g.bfv_compose(L, size, n, dw, At(back, N))
                assert np.array_equal(inner_of(back, N, what).reshape(n, size, L, N), np_compose(words, o.moduli, o.t, size, L)), (what, "masked sum")
                for b in (dx, buf, back, dw):
                    b.free()
    g.close()


def composition(g, L, size, n, dx, L_out, F, N):
    """the definition: he355_bfv_decompose, then he355_bfv_plain_to_ntt"""
    plain, ref = g.alloc(n * F * N), g.alloc(n * F * L_out * N)
    g.bfv_decompose(L, size, n, dx, plain)
    g.bfv_plain_to_ntt(L_out, n * F, plain, ref)
    out = ref.download((n, F, L_out, N))
    plain.free()
    ref.free()
    return out


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_decompose_ntt_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(74)
    for L in sorted({g.L, 1}):
        total, _ = g.bfv_digit_count(L)
        for L_out in sorted({g.L, 1}):
            for size in (2, 3):
                F = size * total
                for n in (1, 3):
                    what = (L, L_out, size, n)
                    x = edged(o, rng, n, L, size)
                    dx = g.to_device(x)
                    want = composition(g, L, size, n, dx, L_out, F, N)
                    buf = sentinelled(g, n * F * L_out * N, N)
                    g.bfv_decompose_ntt(L, size, n, dx, L_out, At(buf, N))
                    assert np.array_equal(inner_of(buf, N, what).reshape(n, F, L_out, N), want), what
                    assert np.array_equal(dx.download((n, size, L, N)), x), (what, "input")
                    dx.free()
                    buf.free()
    # behind an unsynchronised producer: x = a + b is still being written when the call is queued
    L, L_out, size, n = g.L, g.L, 2, 3
    F = size * g.bfv_digit_count(L)[0]
    x, b = edged(o, rng, n, L, size), rand_cts(o, rng, n, L, size)
    a = np.empty_like(x)
    for i, q in enumerate(o.moduli[:L]):
        q = np.uint64(q)
        a[:, :, i] = np.where(x[:, :, i] >= b[:, :, i], x[:, :, i] - b[:, :, i], x[:, :, i] + (q - b[:, :, i]))
    da, db, dx, out = g.to_device(a), g.to_device(b), g.to_device(np.zeros_like(x)), g.alloc(n * F * L_out * N)
    g.sync()
    g.add(L, size, n, da, db, be.Context.pairwise(), dx)
    g.bfv_decompose_ntt(L, size, n, dx, L_out, out)
    got = out.download((n, F, L_out, N))
    assert np.array_equal(dx.download((n, size, L, N)), x)
    assert np.array_equal(got, composition(g, L, size, n, dx, L_out, F, N)), "producer"
    g.close()


def test_refusals(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    rng = np.random.default_rng(75)
    L = g.L
    total, _ = g.bfv_digit_count(L)
    F = 2 * total
    x = rand_cts(o, rng, 2, L)
    dx = g.to_device(x)
    out = g.to_device(np.full(2 * F * L * N, SENT, dtype=np.uint64))
    dec = lambda L_=L, size=2, n=2, src=dx, dst=out: g.bfv_decompose(L_, size, n, src, dst)
    ntt = lambda L_=L, size=2, n=2, src=dx, L_out=L, dst=out: g.bfv_decompose_ntt(L_, size, n, src, L_out, dst)
    com = lambda L_=L, size=2, n=2, src=dx, dst=out: g.bfv_compose(L_, size, n, src, dst)
    for f in (dec, ntt, com):
        refused(be, lambda: f(size=0))
        refused(be, lambda: f(size=4))
        refused(be, lambda: f(L_=0))
        refused(be, lambda: f(L_=L + 1))
        refused(be, lambda: f(src=out))                  # the same slab
        refused(be, lambda: f(src=At(out, N), n=1))      # the input inside the output
        refused(be, lambda: f(n=2 ** 32))                # n F above 2^32 - 1
        f(n=0)
    refused(be, lambda: ntt(L_out=0))
    refused(be, lambda: ntt(L_out=L + 1))
    # the output's last polynomial runs into the input: one slab, the input N words before the end of the output's range
    per_ct, per_pl = 2 * L * N, F * N
    slab = g.to_device(np.full(per_pl + per_ct, SENT, dtype=np.uint64))
    refused(be, lambda: g.bfv_decompose(L, 2, 1, At(slab, per_pl - N), slab))
    refused(be, lambda: g.bfv_compose(L, 2, 1, slab, At(slab, per_pl - N)))
    # the same at L = 1 -> L_out = 1, where F is the level's own and smaller
    per_pl1 = 2 * g.bfv_digit_count(1)[0] * N
    assert per_pl1 < per_pl
    refused(be, lambda: g.bfv_decompose_ntt(1, 2, 1, At(slab, per_pl1 - N), 1, slab))
    # and at L_out = L_top, where the output's range is L_top times as long: the input starts inside its last polynomial
    assert per_pl1 * L + N <= per_pl + per_ct  # the input's 2 N words still lie inside the slab
    refused(be, lambda: g.bfv_decompose_ntt(1, 2, 1, At(slab, per_pl1 * L - N), L, slab))
    assert (slab.download() == SENT).all()
    assert (out.download() == SENT).all()
    assert np.array_equal(dx.download((2, 2, L, N)), x)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(2 * L * N), ck.to_device(np.full(F * L * N, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_decompose(ck.L, 2, 1, a, b))
    refused(be, lambda: ck.bfv_decompose_ntt(ck.L, 2, 1, a, ck.L, b))
    refused(be, lambda: ck.bfv_compose(ck.L, 2, 1, b, a))
    assert ck.bfv_digit_count(1) == (0, [])
    assert (b.download() == SENT).all()
    ck.close()


def test_end_to_end_two_dimensional_retrieval(be, oracle):
    n1 = n2 = 8
    count, n, idx = n1 + n2, 2, [(5, 2), (0, 7)]
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    expand_keys(g, o, sk, count, 160)
    L, t = g.L, o.t
    assert L == 3
    rng = np.random.default_rng(76)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)  # full-range plaintexts
    db[5, 2, :4] = [0, 1, t - 1, t // 2]
    qp = np.zeros((n, N), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = qp[r, n1 + j] = pow(16, -1, t)
    per = 2 * L * N
    budgets = {}
    query, kids = g.alloc(n * per), g.alloc(count * n * per)
    g.encrypt(n, g.to_device(qp), 94, 0, query)
    budgets["fresh"] = g.bfv_noise_budget(L, 2, n, query)
    g.bfv_expand(L, n, query, count, kids)                                                   # 1
    budgets["expand"] = g.bfv_noise_budget(L, 2, count * n, kids)
    g.bfv_transform_to_ntt(L, 2, count * n, kids, kids)                                      # 2
    dbn = g.alloc(n1 * n2 * L * N)
    g.bfv_plain_to_ntt(L, n1 * n2, g.to_device(db.reshape(n1 * n2, N)), dbn)
    res1 = g.alloc(n * n2 * per)
    g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)           # 3: result (r, j) = Enc(db[i_r][j])
    g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)                                       # 4
    budgets["scan 1 (L = 3)"] = g.bfv_noise_budget(L, 2, n * n2, res1)
    Ld = 1
    low = g.alloc(n * n2 * 2 * Ld * N)
    g.bfv_mod_switch(L, Ld, 2, n * n2, res1, low)                                            # 5
    budgets["mod switch (L = 1)"] = g.bfv_noise_budget(Ld, 2, n * n2, low)
    F = 2 * g.bfv_digit_count(Ld)[0]
    cut = g.alloc(n * n2 * F * L * N)
    g.bfv_decompose_ntt(Ld, 2, n * n2, low, L, cut)                                          # 6: plaintext (r n2 + j) F + f
    res2 = g.alloc(n * F * per)
    for r in range(n):                                                                       # 7: result (r, f) = Enc(digit f of Enc(db[i_r][j_r]))
        g.bfv_multiply_plain_accumulate(L, 2, 1, F, n2, At(kids, (n1 * n + r) * per), 1, n, At(cut, r * n2 * F * L * N), F, 1, At(res2, r * F * per))
    g.bfv_transform_from_ntt(L, 2, n * F, res2, res2)                                        # 8
    budgets["scan 2 (L = 3)"] = g.bfv_noise_budget(L, 2, n * F, res2)
    pieces = g.alloc(n * F * N)
    g.decrypt(L, 2, n * F, res2, pieces)                                                     # 9
    glued = g.alloc(n * 2 * Ld * N)
    g.bfv_compose(Ld, 2, n, pieces, glued)                                                   # 10
    budgets["composed (L = 1)"] = g.bfv_noise_budget(Ld, 2, n, glued)
    final = g.alloc(n * N)
    g.decrypt(Ld, 2, n, glued, final)                                                        # 11
    print("two-dimensional retrieval: noise budgets (bits) " + ", ".join(f"{k} {v.min()}..{v.max()}" for k, v in budgets.items()))
    for k, v in budgets.items():
        assert (v > 0).all(), (k, v)
    # the glued ciphertext IS the first scan's result at L = 1, bit for bit
    assert np.array_equal(glued.download((n, 2, Ld, N)), low.download((n * n2, 2, Ld, N))[[r * n2 + j for r, (_, j) in enumerate(idx)]])
    assert np.array_equal(final.download((n, N)), np.stack([db[i, j] for i, j in idx]))
    g.close()


@pytest.mark.parametrize("chain", ["n1024", "n4096_d3"])
def test_second_identical_decompose_ntt_makes_no_raw_allocation(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(77)
    L, size, n = 1, 2, 3
    F = size * g.bfv_digit_count(L)[0]
    x = rand_cts(o, rng, n, L, size)
    dx, out = g.to_device(x), g.alloc(n * F * g.L * N)
    g.bfv_decompose_ntt(L, size, n, dx, g.L, out)
    g.sync()
    first = g.alloc_stats()
    g.bfv_route_stats(reset=True)
    g.bfv_decompose_ntt(L, size, n, dx, g.L, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    routes = {k: c for k, c in g.bfv_route_stats().items() if c}  # N = 1024 has no column pass and takes the composition
    assert routes == ({"digits_routed": 1} if N == 1024 else {"digits_fused": 1}), routes
    assert np.array_equal(out.download((n, F, g.L, N)), composition(g, L, size, n, dx, g.L, F, N))
    g.close()
