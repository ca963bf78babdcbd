"""GPU parity of the BFV selection tree he355_bfv_select, bit-exact (np.array_equal, no tolerance).  Chains, as in
test_gpu_bfv_external_product.py: n1024 (Shoup form, no column pass: the routed tail and the streaming cut), (2048, {60, 40, 60}) (the smallest
column pass, both engines) and n4096_d3 (fold form).

* against the composition of the public calls, level by level: he355_sub of the gathered odd and even nodes, he355_bfv_external_product with
  inner 1 (one call per result, that result's selector of the level shared by its pairs), he355_add of the even nodes, the node without a
  partner copied.  Uniform "RGSW" slabs (the identity is arithmetic), edged leaves.  count in {1, 2, 3, 5, 8} x n in {1, 3} x L in {L_top, 1},
  with BOTH selector layouts where they differ (n = 3: one set of bits for all results, rg_stride_r = 0, and one per result), each case with a
  digit width and a leaf layout (row-major (count, 1), child-major (1, n), padded (count + 1, 1)) taken in turn; then count = 5, n = 3
  under every v in {4, 20, 45, 63} x L in {L_top, 1}, and under every leaf layout x selector layout.  Sentinels around the output, the leaves
  and selectors read back unchanged; once more behind an unsynchronised he355_add; a second identical call makes no raw allocation;
* both cuts in one call: L = 2, n = 4, count = 8 -- level 0 has 16 pairs, 256 column-pass blocks, levels 1 and 2 are below that: select_cols
  1, select_stream 2 where the ring has a column pass (3 streaming cuts at N = 1024), the tail counters per chain; n = 1 makes the last level
  one pair, k_bfv_plain_mac's;
* two passes, the last one ragged: the 2048 chain at L = 1, v = 4 has 2E = 30 terms, a pass of 4096 // 30 = 136 pairs; count = 2 and n = 137;
  and n1024 at L = 1, v = 4 (2E = 26, a pass of 157 pairs, n = 158), where the two passes share the level's one routed tail;
* more terms than a run: n4096_d3, L = 3, v = 1, count = 3, n = 2 -- 2E = 280 is above the 256-term run of the 60-bit prime, a fold happens;
* meaning, real keys, n4096_d3, v = 20, L = L_top: 8 leaves of full-range plaintexts and he355_bfv_rgsw_encrypt of each bit; all 8 bit vectors
  decrypt to leaf sum b_j 2^j, and count = 5 to the leaf tests/bfv_select_ref.py names for every bit vector.  The budget is positive (printed):
  three levels of 14 rows x N = 4096 x digits below 2^20 x fresh noise 2^17.3 add at most about 2^54.7 against 2^(140 - 20 - 1);
* end to end on the database and queries of test_gpu_bfv_selectors.py::test_end_to_end_one_ciphertext_per_query (8 x 8, two queries): three bit
  selectors packed with he355_bfv_selector_encrypt (count = 8 + 3 * 7 = 29, d = 5): expand -> scan -> he355_bfv_rgsw_from_bfv of 21 children ->
  he355_bfv_select -> mod-switch to L = 1 -> one decrypt per query gives db[i][j]; the budget is positive after every stage and printed next
  to the one-hot route's stages (8 selectors, count = 64, d = 6, he355_bfv_external_product) from the same run; nothing is asserted on the
  difference;
* refusals with a device context: a bad L, v, count, strides and overlaps leave the output sentinel-clean; n == 0 touches nothing; count == 1
  copies."""
import itertools

import numpy as np
import pytest

import bfv_select_ref as ref
from bfv_gpu_helpers import SENT, At, be, edged, expand_keys, inner_of, pair, rand_cts, refused, routes, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
CHAINS = ["n1024", N2048, "n4096_d3"]
IDS = ["n1024", "n2048", "n4096_d3"]
WIDTHS = (4, 20, 45, 63)
LAYOUTS = ("row-major", "child-major", "padded")


def leaf_strides(layout, n, count):
    return {"row-major": (count, 1), "child-major": (1, n), "padded": (count + 1, 1)}[layout]


def composition(be, g, L, v, n, count, x, sr, sk, rg, rr, rj, rows, N):
    """the definition with the public calls; x: the leaf slab on the host [.][2][L][N].  Returns [n][2][L][N]"""
    per = 2 * L * N
    pw = be.Context.pairwise()
    nodes = [[x[r * sr + k * sk] for k in range(count)] for r in range(n)]
    j = 0
    while len(nodes[0]) > 1:
        c = len(nodes[0])
        pairs = c // 2
        de = g.to_device(np.stack([nodes[r][2 * p] for r in range(n) for p in range(pairs)]))
        do = g.to_device(np.stack([nodes[r][2 * p + 1] for r in range(n) for p in range(pairs)]))
        diff, pick, nxt = g.alloc(n * pairs * per), g.alloc(n * pairs * per), g.alloc(n * pairs * per)
        g.add(L, 2, n * pairs, do, de, pw, diff, sub=True)
        for r in range(n):  # the pairs of result r share RGSW (r, j)
            g.bfv_external_product(L, v, pairs, 1, At(diff, r * pairs * per), 1, 1, At(rg, (r * rr + j * rj) * rows * per), 0, 1, At(pick, r * pairs * per))
        g.add(L, 2, n * pairs, de, pick, pw, nxt)
        got = nxt.download((n, pairs, 2, L, N))
        nodes = [[got[r, p] for p in range(pairs)] + ([nodes[r][c - 1]] if c & 1 else []) for r in range(n)]
        for b in (de, do, diff, pick, nxt):
            b.free()
        j += 1
    return np.stack([nodes[r][0] for r in range(n)])


def select_case(be, g, o, rng, L, v, n, count, shared, layout, N, what, routed=None, producer=False, twice=False):
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    per = 2 * L * N
    m = ref.depth(count)
    sr, sk = leaf_strides(layout, n, count)
    span = (n - 1) * sr + (count - 1) * sk + 1
    rr, rj = (0, 1) if shared else (m, 1)
    n_rg = max(1, m if shared else n * m)
    rg = g.alloc(n_rg * rows * per)
    g.fill_uniform(rg, n_rg * rows * 2 * L, list(range(L)), 3000 + 16 * n + count + v)
    rg_before = rg.download()
    x = edged(o, rng, span, L)
    if producer:  # x = a + b is still being written when the call is queued
        b = rand_cts(o, rng, span, L)
        a = np.empty_like(x)
        for i, q in enumerate(o.moduli[:L]):
            q = np.uint64(q)
            a[:, :, i] = np.where(x[:, :, i] >= b[:, :, i], x[:, :, i] - b[:, :, i], x[:, :, i] + (q - b[:, :, i]))
        da, db, dx = g.to_device(a), g.to_device(b), g.to_device(np.zeros_like(x))
    else:
        dx = g.to_device(x)
    buf = sentinelled(g, n * per, N)
    g.sync()
    g.bfv_route_stats(reset=True)
    if producer:
        g.add(L, 2, span, da, db, be.Context.pairwise(), dx)
    g.bfv_select(L, v, n, count, dx, sr, sk, rg, rr, rj, At(buf, N))
    if routed is not None:
        assert routes(g) == routed, (what, routes(g))
    got = inner_of(buf, N, what).reshape(n, 2, L, N)
    want = composition(be, g, L, v, n, count, x, sr, sk, rg, rr, rj, rows, N)
    assert np.array_equal(got, want), what
    assert np.array_equal(dx.download(x.shape), x), (what, "leaves")
    assert np.array_equal(rg.download(), rg_before), (what, "selectors")
    if twice:  # a second identical call makes no raw allocation
        g.sync()
        first = g.alloc_stats()
        g.bfv_select(L, v, n, count, dx, sr, sk, rg, rr, rj, At(buf, N))
        g.sync()
        second = g.alloc_stats()
        assert (second["raw_mallocs"], second["raw_frees"]) == (first["raw_mallocs"], first["raw_frees"]), (first, second)
        assert np.array_equal(inner_of(buf, N, what).reshape(n, 2, L, N), want), (what, "again")
    for b in (rg, dx, buf):
        b.free()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_select_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(120)
    # (L, n, selector layout) makes 6 combinations, both selector layouts where they differ (n = 3); combination k runs count number ci with
    # v = WIDTHS[(k + ci) % 4] and leaf layout LAYOUTS[(k + ci) % 3]: k = 0 .. 5 takes every v and every leaf layout to every count
    combos = [(L, n, shared) for L in sorted({g.L, 1}) for n in (1, 3) for shared in ((True,) if n == 1 else (True, False))]
    assert len(combos) == (6 if g.L > 1 else 3)
    for k, (L, n, shared) in enumerate(combos):
        for ci, count in enumerate((1, 2, 3, 5, 8)):
            v, layout = WIDTHS[(k + ci) % 4], LAYOUTS[(k + ci) % 3]
            select_case(be, g, o, rng, L, v, n, count, shared, layout, N, (L, v, n, count, shared, layout))
    for L in sorted({g.L, 1}):
        for v in WIDTHS:
            select_case(be, g, o, rng, L, v, 3, 5, v in (4, 45), "row-major", N, (L, v, "widths"))
    for layout in LAYOUTS:
        for shared in (True, False):
            select_case(be, g, o, rng, g.L, 20, 3, 5, shared, layout, N, (layout, shared, "layouts"))
            select_case(be, g, o, rng, g.L, 20, 3, 8, shared, layout, N, (layout, shared, "layouts, 8"))
    select_case(be, g, o, rng, g.L, 20, 3, 5, False, "child-major", N, "producer", producer=True)
    select_case(be, g, o, rng, g.L, 20, 3, 5, False, "padded", N, "twice", twice=True)
    g.close()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_both_cuts_in_one_call(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(121)
    L, v, count = 2, 20, 8
    assert g.L >= 2 and 4096 // (2 * g.bfv_gadget_count(L, v)[0]) >= 16  # one pass per level
    cols = N > 1024
    tail = {"select_tail_fused": 3} if cols else {"select_tail_routed": 3}
    cuts = {"select_cols": 1, "select_stream": 2} if cols else {"select_stream": 3}
    # n = 4: 16, 8 and 4 pairs; 16 pairs x 2 polynomials x 2 primes x 4 blocks = 256, the threshold
    select_case(be, g, o, rng, L, v, 4, count, False, "row-major", N, (chain, 4), {**cuts, **tail, "passes": 3, "mac_gadget": 3})
    # n = 1: 4, 2 and 1 pairs, all below the threshold; the last level is one pair
    select_case(be, g, o, rng, L, v, 1, count, False, "row-major", N, (chain, 1), {"select_stream": 3, **tail, "passes": 3, "mac_gadget": 2, "mac_plain": 1})
    g.close()


def test_two_passes_the_last_one_ragged(be, oracle):
    g, o, N, *_ = pair(be, oracle, N2048)
    L, v, count = 1, 4, 2
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    assert rows == 30
    n = 4096 // rows + 1  # the plan's pass (bfv_gadget_pass over 2E terms) holds 136 pairs: the smallest n that needs two
    assert n == 137
    # 136 pairs: 1088 column-pass blocks; the last pair alone streams
    select_case(be, g, o, np.random.default_rng(122), L, v, n, count, True, "row-major", N, "two passes",
                {"select_cols": 1, "select_stream": 1, "select_tail_fused": 1, "passes": 2, "mac_gadget": 2})
    g.close()


def test_two_passes_at_n1024_share_one_tail(be, oracle):
    """N = 1024 runs its routed tail once per level, over the sums of all passes: two passes, the last one ragged, one tail"""
    g, o, N, *_ = pair(be, oracle, "n1024")
    L, v, count = 1, 4, 2
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    assert rows == 26  # a 50-bit prime in 4-bit digits
    n = 4096 // rows + 1
    assert n == 158
    select_case(be, g, o, np.random.default_rng(126), L, v, n, count, True, "row-major", N, "two passes, n1024",
                {"select_stream": 2, "select_tail_routed": 1, "passes": 2, "mac_gadget": 2})
    g.close()


def test_more_terms_than_a_run(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    L, v = 3, 1
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    run = (2 ** 128 - 1) // (o.moduli[0] - 1) ** 2
    assert rows == 280 and o.moduli[0].bit_length() == 60 and run == 256 and rows > run
    select_case(be, g, o, np.random.default_rng(123), L, v, 2, 3, True, "row-major", N, "fold",
                {"select_stream": 2, "select_tail_fused": 2, "passes": 2, "mac_gadget": 2})
    g.close()


def test_meaning_with_real_keys(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(124)
    L, v, t = g.L, 20, o.t
    rows = 2 * g.bfv_gadget_count(L, v)[0]
    assert rows == 14
    per = 2 * L * N
    mu = rng.integers(0, t, (8, N), dtype=np.uint64)
    mu[0, :4] = [0, 1, t - 1, t // 2]
    leaves = g.alloc(8 * per)
    g.encrypt(8, g.to_device(mu), 130, 0, leaves)
    vectors = list(itertools.product((0, 1), repeat=3))  # (b_0, b_1, b_2)
    bits = np.zeros((len(vectors) * 3, N), dtype=np.uint64)
    for i, bv in enumerate(vectors):
        bits[3 * i:3 * i + 3, 0] = bv
    rg = g.alloc(len(vectors) * 3 * rows * per)
    g.bfv_rgsw_encrypt(L, v, len(vectors) * 3, g.to_device(bits), 131, 0, rg)
    out, dec = g.alloc(per), g.alloc(N)
    fresh = int(g.bfv_noise_budget(L, 2, 8, leaves).min())
    low = {}
    for count in (8, 5):
        for i, bv in enumerate(vectors):
            g.bfv_select(L, v, 1, count, leaves, count, 1, At(rg, 3 * i * rows * per), 0, 1, out)
            budget = int(g.bfv_noise_budget(L, 2, 1, out)[0])
            low[count] = min(low.get(count, budget), budget)
            assert budget > 0, (count, bv, budget)
            g.decrypt(L, 2, 1, out, dec)
            leaf = ref.selected_leaf(count, bv)
            if count == 8:
                assert leaf == sum(b << j for j, b in enumerate(bv))
            assert np.array_equal(dec.download(), mu[leaf]), (count, bv, leaf)
    print(f"selection tree (L = {L}, v = {v}): noise budget {fresh} fresh, at least {low[8]} after 8 leaves, {low[5]} after 5")
    g.close()


def test_end_to_end_bit_selectors_in_one_query(be, oracle):
    n1 = n2 = 8
    n, idx = 2, [(5, 2), (0, 7)]
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    L, t, v, kv = g.L, o.t, 20, 20
    assert L == 3
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    expand_keys(g, o, sk, 64, 180)  # the keys of d = 6 hold those of d = 5
    rng = np.random.default_rng(76)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)  # the database of test_gpu_bfv_selectors.py
    db[5, 2, :4] = [0, 1, t - 1, t // 2]
    per = 2 * L * N
    pw = be.Context.pairwise()
    dbn = g.alloc(n1 * n2 * L * N)
    g.bfv_plain_to_ntt(L, n1 * n2, g.to_device(db.reshape(n1 * n2, N)), dbn)
    key = g.alloc(rows * per)
    g.bfv_rgsw_encrypt_secret(L, kv, 96, 0, key)

    def retrieve(n_sel, sel, fold):
        """one query ciphertext per retrieval with n_sel packed selectors; fold(res1, rg, one): the second dimension"""
        count = n1 + n_sel * E
        d = ref.depth(count)
        qp = np.zeros((n, N), dtype=np.uint64)
        for r, (i, _) in enumerate(idx):
            qp[r, i] = pow(1 << d, -1, t)
        budgets = {}
        first_dim, packed, query = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
        g.encrypt(n, g.to_device(qp), 94, 0, first_dim)
        budgets["fresh"] = g.bfv_noise_budget(L, 2, n, first_dim)
        g.bfv_selector_encrypt(L, v, n, n_sel, n1, count, g.to_device(sel), 95, 0, packed)
        g.add(L, 2, n, first_dim, packed, pw, query)
        kids = g.alloc(count * n * per)
        g.bfv_expand(L, n, query, count, kids)                                               # 1: child k of query r at k n + r
        budgets["expand"] = g.bfv_noise_budget(L, 2, n1 * n, kids)
        g.bfv_transform_to_ntt(L, 2, n1 * n, kids, kids)
        res1 = g.alloc(n * n2 * per)
        g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)       # 2: result (r, j) = Enc(db[i_r][j])
        g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)
        budgets["scan"] = g.bfv_noise_budget(L, 2, n * n2, res1)
        rg = g.alloc(n * n_sel * 2 * E * per)
        g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, At(kids, n1 * n * per), 1, n, key, rg)       # 3: n_sel E children per query -> RGSW (r, b)
        one = g.alloc(n * per)
        fold(res1, rg, one)                                                                  # 4: ONE ciphertext per query
        budgets["second dimension"] = g.bfv_noise_budget(L, 2, n, one)
        low = g.alloc(n * 2 * N)
        g.bfv_mod_switch(L, 1, 2, n, one, low)                                               # 5
        budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, n, low)
        final = g.alloc(n * N)
        g.decrypt(1, 2, n, low, final)                                                       # 6: one decrypt per query
        for b in (first_dim, packed, query, kids, res1, rg, one, low):
            b.free()
        return count, d, n_sel * E, budgets, final.download((n, N))

    bit_sel = np.array([[(j >> b) & 1 for b in range(3)] for _, j in idx], dtype=np.uint64)
    hot_sel = np.zeros((n, n2), dtype=np.uint64)
    for r, (_, j) in enumerate(idx):
        hot_sel[r, j] = 1
    want = np.stack([db[i, j] for i, j in idx])
    tree = retrieve(3, bit_sel, lambda res1, rg, one: g.bfv_select(L, v, n, n2, res1, n2, 1, rg, 3, 1, one))
    hot = retrieve(n2, hot_sel, lambda res1, rg, one: g.bfv_external_product(L, v, n, n2, res1, n2, 1, rg, n2, 1, one))
    assert tree[:3] == (29, 5, 21) and hot[:3] == (64, 6, 56)
    for name, (count, d, conv, budgets, got) in (("3 bit selectors, he355_bfv_select", tree), ("8 one-hot selectors, he355_bfv_external_product", hot)):
        print(f"8 x 8 retrieval, {name}: {count} children expanded (d = {d}), {conv} converted; noise budgets (bits) "
              + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in budgets.items()))
        for k, b in budgets.items():
            assert (b > 0).all(), (name, k, b)
        assert np.array_equal(got, want), name
    g.close()


def test_refusals_and_trivial_calls(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    rng = np.random.default_rng(125)
    L, v = g.L, 20
    rows, per = 2 * g.bfv_gadget_count(L, v)[0], 2 * L * N
    x = rand_cts(o, rng, 8, L)
    dx = g.to_device(x)
    rgs = g.to_device(np.full(2 * rows * per, SENT, dtype=np.uint64))
    out = g.to_device(np.full(4 * per, SENT, dtype=np.uint64))
    sel = lambda L_=L, w=v, n=2, count=4, ct=dx, sr=4, sk=1, rg=rgs, rr=0, rj=1, dst=out: g.bfv_select(L_, w, n, count, ct, sr, sk, rg, rr, rj, dst)
    for bad in (dict(L_=0), dict(L_=L + 1), dict(w=0), dict(w=64), dict(count=0), dict(count=2 ** 24 + 1), dict(sk=0), dict(sr=0), dict(sr=1, sk=1),
                dict(sr=2 ** 60), dict(rj=2 ** 60), dict(n=2 ** 31), dict(dst=dx), dict(dst=At(dx, 8 * per - 1)), dict(dst=rgs),
                dict(dst=At(rgs, 2 * rows * per - 1), n=1), dict(count=1, n=1, dst=At(dx, N))):
        refused(be, lambda: sel(**bad))
    # n == 0 touches nothing, whatever else is passed
    sel(n=0, sr=0, sk=0, dst=dx)
    assert (out.download() == SENT).all() and (rgs.download() == SENT).all()
    assert np.array_equal(dx.download(x.shape), x)
    # count == 1 copies leaf (r, 0), through the strides, and reads no selector
    buf = sentinelled(g, 3 * per, N)
    g.bfv_route_stats(reset=True)
    sel(n=3, count=1, sr=3, sk=0, dst=At(buf, N))
    assert routes(g) == {}
    assert np.array_equal(inner_of(buf, N, "count 1").reshape(3, 2, L, N), x[[0, 3, 6]])
    assert np.array_equal(dx.download(x.shape), x) and (rgs.download() == SENT).all()
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(4 * per), ck.to_device(np.full(per, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_select(1, v, 1, 2, a, 2, 1, a, 0, 1, b))
    assert (b.download() == SENT).all()
    ck.close()
