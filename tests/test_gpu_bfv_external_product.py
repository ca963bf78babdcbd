"""GPU parity of the BFV external product RGSW(m) [.] BFV(mu) -> BFV(m mu) (he355_bfv_gadget_count, he355_bfv_gadget_decompose,
he355_bfv_gadget_decompose_ntt, he355_bfv_rgsw_encrypt, he355_bfv_external_product), bit-exact (np.array_equal, no tolerance).  Chains: n1024
(Shoup form, no column pass), (2048, {60, 40, 60}) (the smallest column pass) and n4096_d3 (fold form, both engines).

* gadget_decompose against numpy: v in {4, 20, 45, 63} (45 lies between the 40- and 60-bit primes; 63 gives E_i = 1), L in {L_top, 1}, sizes
  1..3, n in {1, 3}; uniform rows mixed with all-0, all-(q - 1) and alternating rows; sentinels around the output, the input read back;
* gadget_decompose_ntt == gadget_decompose, the digits under every prime (reduced where not below it), he355_ntt_forward: the same grid, and
  n size L = 62, 64 and 198 (N >= 2048 runs the column pass from 256 blocks = n size L of 64 on, N = 1024's route below); once more behind
  an unsynchronised he355_add; a second identical call makes no raw allocation; the routes are bit-identical, so the 62 / 64 / 198 cases and the
  run-boundary cases also assert he355_bfv_route_stats (which cut, which multiply-accumulate kernel, how many passes);
* rgsw_encrypt == encrypt_zero with the same seed and indices, cut to L, the planted term in numpy, he355_bfv_transform_to_ntt: L in
  {L_top, 1}, messages 0, 1, X^5, -X^(N-1) and full-range;
* external_product == gadget_decompose_ntt of the inner ciphertexts + he355_bfv_multiply_plain_accumulate(L, 2, 1, 1, inner 2E) with the RGSW
  rows as the ciphertext operand + he355_bfv_transform_from_ntt, per result: uniform "RGSW" slabs (the identity is arithmetic), edged
  ciphertexts, n and inner in {1, 3} (n = 1 runs the composition's own inner product) and 6 x 3 (enough ciphertexts for the column pass), one
  selector row for all results (rg_stride_r = 0) and one per result, child-major ciphertexts (non-unit ct_stride_k) at 3 x 3 and at 6 x 3,
  where the column pass itself reads at the strides; the run boundary on the 2048 chain at L = 1, v = 4: inner = 9 is 270 terms, above the
  256-term run of the 60-bit prime (a fold happens; 16 results there also make the call take two passes through its pool block), inner = 8 is 240 (no fold); sentinels, operands read back;
* meaning, real keys, n4096_d3, v = 20: decrypt(external_product(RGSW(m), Enc(mu))) == m mu in Z_t[X]/(X^N + 1) by Python integers, m in
  {0, 1, X^7, t - 1}, mu full-range; the noise budget is positive (printed);
* end to end on the 8 x 8 database and the two queries of test_gpu_bfv_digits.py: expand(8) -> to_ntt -> first scan -> from_ntt -> mod_switch
  to L = 2 -> external product at L = 2, v = 20, inner = 8 with RGSW(delta_(j, j*)) per column, one selector row per query (rg_stride_r = 8) ->
  mod_switch to L = 1 -> ONE decrypt per query gives db[i][j]; the budget is positive after every stage (printed).  The margin at L = 2 is
  derived: 2E = 10 rows x inner 8, N = 4096, digits below 2^20 and fresh noise at most 2 N 19.2 ~ 2^17.3 add at most ~ 2^55.6 against
  2^(100 - 20 - 1), about 23 bits in the worst case.  (Not run at L = 1: the same bound does not guarantee a positive budget there.)
* a two-level selection tree over 4 ciphertexts (he355_sub, external product with RGSW(bit), he355_add, twice) decrypts to the chosen one for
  all four bit pairs: outputs chain as inputs;
* refusals: a CKKS context, a bad L, a bad v, size 0 / 4, inner == 0, every overlap, rgsw_encrypt without a public key -- the code, a message,
  the output sentinel-clean; n == 0 touches nothing."""
import ctypes as C

import numpy as np
import pytest

import bfv_gadget_ref as ref
from bfv_gpu_helpers import SENT, At, be, edged, ep_composition, expand_keys, inner_of, pair, rand_cts, refused, routes, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
CHAINS = ["n1024", N2048, "n4096_d3"]
IDS = ["n1024", "n2048", "n4096_d3"]
WIDTHS = (4, 20, 45, 63)


def ntt_forward(be, g, buf, n_polys, L):
    """he355_ntt_forward of [n_polys / L][L][N], polynomial p under prime p % L"""
    pm = (C.c_uint8 * L)(*range(L))
    assert be.lib().he355_ntt_forward(g.h, buf.ptr, n_polys, pm, L) == 0


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_gadget_decompose_against_numpy(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(83)
    for L in sorted({g.L, 1}):
        for v in WIDTHS:
            E, off = ref.table(o.moduli[:L], v)
            assert g.bfv_gadget_count(L, v) == (off[-1], E)
            for size in (1, 2, 3):
                F = size * off[-1]
                for n in (1, 3):
                    what = (L, v, size, n)
                    x = edged(o, rng, n, L, size)
                    dx = g.to_device(x)
                    buf = sentinelled(g, n * F * N, N)
                    g.bfv_gadget_decompose(L, v, size, n, dx, At(buf, N))
                    assert np.array_equal(inner_of(buf, N, what).reshape(n, F, N), ref.np_digits(x, o.moduli, v)), what
                    assert np.array_equal(dx.download((n, size, L, N)), x), (what, "input")
                    dx.free()
                    buf.free()
    g.close()


def composition_ntt(be, g, o, L, v, size, n, dx, F, N):
    """the definition: he355_bfv_gadget_decompose, every digit polynomial under every prime j < L, he355_ntt_forward"""
    dig = g.alloc(n * F * N)
    g.bfv_gadget_decompose(L, v, size, n, dx, dig)
    d = dig.download((n, F, N))
    dig.free()
    wide = g.to_device(ref.np_spread(d, o.moduli[:L]))
    ntt_forward(be, g, wide, n * F * L, L)
    out = wide.download((n, F, L, N))
    wide.free()
    return out


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_gadget_decompose_ntt_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(84)
    for L in sorted({g.L, 1}):
        for v in WIDTHS:
            total = g.bfv_gadget_count(L, v)[0]
            for size in (1, 2, 3):
                F = size * total
                for n in (1, 3):
                    what = (L, v, size, n)
                    x = edged(o, rng, n, L, size)
                    dx = g.to_device(x)
                    want = composition_ntt(be, g, o, L, v, size, n, dx, F, N)
                    buf = sentinelled(g, n * F * L * N, N)
                    g.bfv_gadget_decompose_ntt(L, v, size, n, dx, At(buf, N))
                    assert np.array_equal(inner_of(buf, N, what).reshape(n, F, L, N), want), what
                    assert np.array_equal(dx.download((n, size, L, N)), x), (what, "input")
                    dx.free()
                    buf.free()
    # N >= 2048: a batch of fewer than 256 column-pass blocks (n size L < 64) takes N = 1024's route; one short of the threshold, at it, above it
    for L, size, n, v in ((1, 2, 31, 20), (1, 2, 32, 20), (g.L, 3, 22, 45)):
        F = size * g.bfv_gadget_count(L, v)[0]
        x = edged(o, rng, n, L, size)
        dx = g.to_device(x)
        buf = sentinelled(g, n * F * L * N, N)
        g.bfv_route_stats(reset=True)
        g.bfv_gadget_decompose_ntt(L, v, size, n, dx, At(buf, N))
        # both routes give the same bits: the counters say which one ran (N = 1024 has no column pass)
        assert routes(g) == ({"cut_cols": 1} if N > 1024 and n * size * L >= 64 else {"cut_stream": 1}), (L, size, n, v)
        assert np.array_equal(inner_of(buf, N, (L, size, n)).reshape(n, F, L, N), composition_ntt(be, g, o, L, v, size, n, dx, F, N)), (L, size, n, v)
        dx.free()
        buf.free()
    # behind an unsynchronised producer: x = a + b is still being written when the call is queued
    L, v, size, n = g.L, 20, 2, 3
    F = size * g.bfv_gadget_count(L, v)[0]
    x, b = edged(o, rng, n, L, size), rand_cts(o, rng, n, L, size)
    a = np.empty_like(x)
    for i, q in enumerate(o.moduli[:L]):
        q = np.uint64(q)
        a[:, :, i] = np.where(x[:, :, i] >= b[:, :, i], x[:, :, i] - b[:, :, i], x[:, :, i] + (q - b[:, :, i]))
    da, db, dx, out = g.to_device(a), g.to_device(b), g.to_device(np.zeros_like(x)), g.alloc(n * F * L * N)
    g.sync()
    g.add(L, size, n, da, db, be.Context.pairwise(), dx)
    g.bfv_gadget_decompose_ntt(L, v, size, n, dx, out)
    got = out.download((n, F, L, N))
    assert np.array_equal(dx.download((n, size, L, N)), x)
    assert np.array_equal(got, composition_ntt(be, g, o, L, v, size, n, dx, F, N)), "producer"
    # a second identical call makes no raw allocation
    g.sync()
    first = g.alloc_stats()
    g.bfv_gadget_decompose_ntt(L, v, size, n, dx, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    assert np.array_equal(out.download((n, F, L, N)), got)
    g.close()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_rgsw_encrypt_equals_the_definition(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    rng = np.random.default_rng(85)
    t, Lt, v, n, seed, first = o.t, g.L, 20, 5, 97, 7
    m = rng.integers(0, t, (n, N), dtype=np.uint64)
    m[0] = 0
    m[1] = 0
    m[1, 0] = 1
    m[2] = 0
    m[2, 5] = 1
    m[3] = 0
    m[3, N - 1] = t - 1
    m[4, :4] = [t // 2, (t + 1) // 2, t - 1, 0]
    dm = g.to_device(m)
    for L in sorted({Lt, 1}):
        rows = 2 * g.bfv_gadget_count(L, v)[0]
        zero = g.alloc(n * rows * 2 * Lt * N)
        g.encrypt_zero(n * rows, seed, first, zero)
        z = zero.download((n, rows, 2, Lt, N))[:, :, :, :L]
        want = g.to_device(np.stack([ref.np_plant(z[r], m[r], o.moduli, t, v) for r in range(n)]))
        g.bfv_transform_to_ntt(L, 2, n * rows, want, want)
        buf = sentinelled(g, n * rows * 2 * L * N, N)
        g.bfv_rgsw_encrypt(L, v, n, dm, seed, first, At(buf, N))
        assert np.array_equal(inner_of(buf, N, L), want.download()), L
        assert np.array_equal(dm.download((n, N)), m)
        g.sync()
        a = g.alloc_stats()
        g.bfv_rgsw_encrypt(L, v, n, dm, seed, first, At(buf, N))  # a second identical call: the pool block and the client arena are there
        g.sync()
        b = g.alloc_stats()
        assert (a["raw_mallocs"], a["raw_frees"]) == (b["raw_mallocs"], b["raw_frees"]), (L, a, b)
        assert np.array_equal(inner_of(buf, N, L), want.download()), (L, "again")
        for x in (zero, want, buf):
            x.free()
    g.close()


def ep_case(g, o, rng, L, v, n, inner, shared, child_major, N, what, routed=None):
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    n_rg = inner if shared else n * inner
    rg = g.alloc(n_rg * rows * per)
    g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 1000 + n * 10 + inner)
    rg_before = rg.download()
    x = edged(o, rng, n * inner, L)
    dx = g.to_device(x)
    sr, sk = (1, n) if child_major else (inner, 1)
    gr = 0 if shared else inner
    want = ep_composition(g, L, v, n, inner, x, lambda r, k: r * sr + k * sk, rg, gr, rows, N)
    buf = sentinelled(g, n * per, N)
    g.bfv_route_stats(reset=True)
    g.bfv_external_product(L, v, n, inner, dx, sr, sk, rg, gr, 1, At(buf, N))
    if routed is not None:
        assert routes(g) == routed, (what, routes(g))
    assert np.array_equal(inner_of(buf, N, what).reshape(n, 2, L, N), want), what
    assert np.array_equal(dx.download(x.shape), x), (what, "ciphertexts")
    assert np.array_equal(rg.download(), rg_before), (what, "RGSW")
    for b in (rg, dx, buf):
        b.free()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_external_product_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(86)
    for L in sorted({g.L, 1}):
        for n in (1, 3):
            for inner in (1, 3):
                for shared in (True, False):
                    ep_case(g, o, rng, L, 20, n, inner, shared, False, N, (L, n, inner, shared))
        ep_case(g, o, rng, L, 20, 3, 3, False, True, N, (L, "child-major"))
        ep_case(g, o, rng, L, 20, 3, 3, True, True, N, (L, "child-major, one selector row"))
        ep_case(g, o, rng, L, 45, 3, 3, False, False, N, (L, "v = 45: digits above the 40-bit primes"))
        ep_case(g, o, rng, L, 63, 2, 3, True, True, N, (L, "v = 63: one digit per prime"))
    for shared in (True, False):  # 18 ciphertexts at L_top: enough blocks for the column pass at N >= 2048 (n = 3 x inner = 3 takes the small-batch route)
        ep_case(g, o, rng, g.L, 20, 6, 3, shared, False, N, (g.L, 6, 3, shared))
        ep_case(g, o, rng, g.L, 20, 6, 3, shared, True, N, (g.L, 6, 3, shared, "child-major"))  # the column pass reads at the strides
    # a second identical call makes no raw allocation
    L, v, n, inner = g.L, 20, 3, 3
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    rg, dx, out = g.alloc(inner * rows * per), g.to_device(edged(o, rng, n * inner, L)), g.alloc(n * per)
    g.fill_uniform(rg, inner * rows * 2 * L, list(range(L)), 5)
    g.bfv_external_product(L, v, n, inner, dx, inner, 1, rg, 0, 1, out)
    g.sync()
    first, got = g.alloc_stats(), out.download()
    g.bfv_external_product(L, v, n, inner, dx, inner, 1, rg, 0, 1, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    assert np.array_equal(out.download(), got)
    g.close()


@pytest.mark.parametrize("inner,n", [(9, 16), (8, 1)], ids=["270_terms_fold_two_passes", "240_terms_no_fold"])
def test_external_product_run_boundary(be, oracle, inner, n):
    g, o, N, *_ = pair(be, oracle, N2048)
    L, v = 1, 4
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    assert rows == 30 and o.moduli[0].bit_length() == 60
    run = (2 ** 128 - 1) // (o.moduli[0] - 1) ** 2
    assert run == 256 and (inner * rows > run) == (inner == 9)
    if n > 1:
        assert 4096 // (inner * rows) < n  # more than one pass through the pool block, the last one ragged
    # 16 results: 15 in the first pass (the column pass), the last one alone (9 ciphertexts: the streaming cut); one result over rows that
    # follow one another is k_bfv_plain_mac's
    routed = {"cut_cols": 1, "cut_stream": 1, "mac_gadget": 2, "passes": 2} if n > 1 else {"cut_stream": 1, "mac_plain": 1, "passes": 1}
    ep_case(g, o, np.random.default_rng(87), L, v, n, inner, True, False, N, (inner, n), routed)
    g.close()


def test_meaning_with_real_keys(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(88)
    L, v, t = g.L, 20, o.t
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    sparse = [{}, {0: 1}, {7: 1}, {0: t - 1}]
    n = len(sparse)
    m = np.zeros((n, N), dtype=np.uint64)
    for r, s in enumerate(sparse):
        for e, c in s.items():
            m[r, e] = c
    mu = rng.integers(0, t, (n, N), dtype=np.uint64)
    mu[0, :4] = [0, 1, t - 1, t // 2]
    rg, ct, out, dec = g.alloc(n * rows * per), g.alloc(n * per), g.alloc(n * per), g.alloc(n * N)
    g.bfv_rgsw_encrypt(L, v, n, g.to_device(m), 101, 0, rg)
    g.encrypt(n, g.to_device(mu), 102, 0, ct)
    g.bfv_external_product(L, v, n, 1, ct, 1, 1, rg, 1, 1, out)
    budget = g.bfv_noise_budget(L, 2, n, out)
    print(f"external product (L = {L}, v = {v}): noise budget {g.bfv_noise_budget(L, 2, n, ct).min()} fresh, {budget.min()}..{budget.max()} after")
    assert (budget > 0).all(), budget
    g.decrypt(L, 2, n, out, dec)
    got = dec.download((n, N))
    for r, s in enumerate(sparse):
        assert np.array_equal(got[r], ref.negacyclic_sparse(mu[r], s, t)), s
    g.close()


def test_end_to_end_two_dimensional_retrieval_one_reply(be, oracle):
    n1 = n2 = 8
    n, idx = 2, [(5, 2), (0, 7)]
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    expand_keys(g, o, sk, n1, 160)
    L, t, v = g.L, o.t, 20
    assert L == 3
    rng = np.random.default_rng(76)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)  # full-range plaintexts
    db[5, 2, :4] = [0, 1, t - 1, t // 2]
    qp = np.zeros((n, N), dtype=np.uint64)
    sel = np.zeros((n, n2, N), dtype=np.uint64)  # RGSW messages: the constant delta_(j, j*)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = pow(n1, -1, t)
        sel[r, j, 0] = 1
    per = 2 * L * N
    budgets = {}
    query, kids = g.alloc(n * per), g.alloc(n1 * n * per)
    g.encrypt(n, g.to_device(qp), 94, 0, query)
    budgets["fresh"] = g.bfv_noise_budget(L, 2, n, query)
    g.bfv_expand(L, n, query, n1, kids)                                                      # 1: child k of query r at k n + r
    budgets["expand"] = g.bfv_noise_budget(L, 2, n1 * n, kids)
    g.bfv_transform_to_ntt(L, 2, n1 * n, kids, kids)                                         # 2
    dbn = g.alloc(n1 * n2 * L * N)
    g.bfv_plain_to_ntt(L, n1 * n2, g.to_device(db.reshape(n1 * n2, N)), dbn)
    res1 = g.alloc(n * n2 * per)
    g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)           # 3: result (r, j) = Enc(db[i_r][j])
    g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)                                       # 4
    budgets["scan 1 (L = 3)"] = g.bfv_noise_budget(L, 2, n * n2, res1)
    Le = 2
    mid = g.alloc(n * n2 * 2 * Le * N)
    g.bfv_mod_switch(L, Le, 2, n * n2, res1, mid)                                            # 5
    budgets["mod switch (L = 2)"] = g.bfv_noise_budget(Le, 2, n * n2, mid)
    rows = 2 * g.bfv_gadget_count(Le, v)[0]
    assert rows == 10
    rg = g.alloc(n * n2 * rows * 2 * Le * N)
    g.bfv_rgsw_encrypt(Le, v, n * n2, g.to_device(sel.reshape(n * n2, N)), 95, 0, rg)        # the client's second-dimension query
    one = g.alloc(n * 2 * Le * N)
    g.bfv_external_product(Le, v, n, n2, mid, n2, 1, rg, n2, 1, one)                         # 6: ONE ciphertext per query
    budgets["external product (L = 2)"] = g.bfv_noise_budget(Le, 2, n, one)
    low = g.alloc(n * 2 * N)
    g.bfv_mod_switch(Le, 1, 2, n, one, low)                                                  # 7
    budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, n, low)
    final = g.alloc(n * N)
    g.decrypt(1, 2, n, low, final)                                                           # 8: one decrypt per query
    print("two-dimensional retrieval, one reply ciphertext: noise budgets (bits) " + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in budgets.items()))
    for k, b in budgets.items():
        assert (b > 0).all(), (k, b)
    assert np.array_equal(final.download((n, N)), np.stack([db[i, j] for i, j in idx]))
    g.close()


def test_two_level_selection_tree(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(89)
    L, v, t = g.L, 20, o.t
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    mu = rng.integers(0, t, (4, N), dtype=np.uint64)
    leaves = g.alloc(4 * per)
    g.encrypt(4, g.to_device(mu), 103, 0, leaves)
    bits = np.zeros((2, N), dtype=np.uint64)
    zero_one = g.alloc(2 * rows * per)  # RGSW(0), RGSW(1)
    bits[1, 0] = 1
    g.bfv_rgsw_encrypt(L, v, 2, g.to_device(bits), 104, 0, zero_one)
    pw = be.Context.pairwise()
    got = {}
    for b1 in (0, 1):
        for b0 in (0, 1):
            # level 1: d_p = c_(2p) + RGSW(b0) [.] (c_(2p+1) - c_(2p)), p = 0, 1, both with the one selector row
            lo = g.to_device(leaves.download((4, 2 * L * N))[[0, 2]])
            hi = g.to_device(leaves.download((4, 2 * L * N))[[1, 3]])
            diff, pick, d = g.alloc(2 * per), g.alloc(2 * per), g.alloc(2 * per)
            g.add(L, 2, 2, hi, lo, pw, diff, sub=True)
            g.bfv_external_product(L, v, 2, 1, diff, 1, 1, At(zero_one, b0 * rows * per), 0, 1, pick)
            g.add(L, 2, 2, lo, pick, pw, d)
            # level 2: out = d_0 + RGSW(b1) [.] (d_1 - d_0): the external product's output is the next one's input as it lies
            diff2, pick2, out = g.alloc(per), g.alloc(per), g.alloc(per)
            g.add(L, 2, 1, At(d, per), d, pw, diff2, sub=True)
            g.bfv_external_product(L, v, 1, 1, diff2, 1, 1, At(zero_one, b1 * rows * per), 0, 1, pick2)
            g.add(L, 2, 1, d, pick2, pw, out)
            budget = g.bfv_noise_budget(L, 2, 1, out)
            assert (budget > 0).all(), (b1, b0, budget)
            dec = g.alloc(N)
            g.decrypt(L, 2, 1, out, dec)
            got[(b1, b0)] = (dec.download(), int(budget[0]))
    print("selection tree: noise budgets " + ", ".join(f"{k} {b}" for k, (_, b) in got.items()))
    for (b1, b0), (m, _) in got.items():
        assert np.array_equal(m, mu[2 * b1 + b0]), (b1, b0)
    g.close()


def test_refusals(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")  # no keys: rgsw_encrypt has no public key
    rng = np.random.default_rng(90)
    L, v = g.L, 20
    E = g.bfv_gadget_count(L, v)[0]
    rows, per = 2 * E, 2 * L * N
    x = rand_cts(o, rng, 2, L)
    dx = g.to_device(x)
    out = g.to_device(np.full(2 * rows * per, SENT, dtype=np.uint64))  # digits, an RGSW ciphertext or results
    rgs = g.to_device(np.full(2 * rows * per, SENT, dtype=np.uint64))
    dec = lambda L_=L, w=v, size=2, n=2, src=dx, dst=out: g.bfv_gadget_decompose(L_, w, size, n, src, dst)
    ntt = lambda L_=L, w=v, size=2, n=2, src=dx, dst=out: g.bfv_gadget_decompose_ntt(L_, w, size, n, src, dst)
    enc = lambda L_=L, w=v, n=1, src=dx, dst=out: g.bfv_rgsw_encrypt(L_, w, n, src, 1, 0, dst)
    ep = lambda L_=L, w=v, n=2, inner=1, ct=dx, sr=1, sk=1, rg=rgs, gr=1, gk=1, dst=out: g.bfv_external_product(L_, w, n, inner, ct, sr, sk, rg, gr, gk, dst)
    for f in (dec, ntt, enc, ep):
        for bad in (dict(L_=0), dict(L_=L + 1), dict(w=0), dict(w=64), dict(w=-1)):
            refused(be, lambda: f(**bad))
        f(n=0)
    for f in (dec, ntt):
        refused(be, lambda: f(size=0))
        refused(be, lambda: f(size=4))
        refused(be, lambda: f(src=out))                  # the same slab
        refused(be, lambda: f(src=At(out, N), n=1))      # the input inside the output
        refused(be, lambda: f(n=2 ** 32))
    refused(be, lambda: enc())                           # valid arguments, no public key
    refused(be, lambda: enc(src=out))
    refused(be, lambda: ep(inner=0))
    refused(be, lambda: ep(inner=2 ** 31))
    refused(be, lambda: ep(ct=out))                      # the output is the ciphertext slab
    refused(be, lambda: ep(ct=At(out, per - 1), n=1))    # ... starts inside it
    refused(be, lambda: ep(rg=out))                      # the output is the RGSW slab
    refused(be, lambda: ep(rg=out, dst=At(out, rows * per - 1), n=1, gr=0))  # ... its last word
    refused(be, lambda: ep(n=1, inner=2, dst=At(dx, per)))                   # the second inner ciphertext
    assert (out.download() == SENT).all() and (rgs.download() == SENT).all()
    assert np.array_equal(dx.download((2, 2, L, N)), x)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(2 * per), ck.to_device(np.full(rows * per, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_gadget_decompose(1, v, 2, 1, a, b))
    refused(be, lambda: ck.bfv_gadget_decompose_ntt(1, v, 2, 1, a, b))
    refused(be, lambda: ck.bfv_rgsw_encrypt(1, v, 1, a, 1, 0, b))
    refused(be, lambda: ck.bfv_external_product(1, v, 1, 1, a, 1, 1, b, 0, 1, At(a, per)))
    assert ck.bfv_gadget_count(1, v) == (0, [])
    assert (b.download() == SENT).all()
    ck.close()
