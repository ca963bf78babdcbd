"""GPU parity of the RGSW selectors packed into ONE query ciphertext (he355_bfv_selector_encrypt, he355_bfv_rgsw_encrypt_secret,
he355_bfv_rgsw_from_bfv), bit-exact (np.array_equal, Python integers, no tolerance).  Chains: n1024 (Shoup form, no column pass),
(2048, {60, 40, 60}) (the smallest column pass) and n4096_d3 (fold form, both engines).

* selector_encrypt == encrypt_zero with the same seed and indices, cut to L, plus the numpy plant (bfv_selector_ref.np_pack): L in {L_top, 1},
  v in {20, 63}, n = 2, n_sel in {1, 3}, first_slot in {0, 5}, count in {first_slot + n_sel E, N}; selectors 0, 1, t - 1 and full-range;
  sentinels around the output, the selectors read back; a second identical call makes no raw allocation;
* rgsw_encrypt_secret == rgsw_encrypt of s mod t, s built here from the oracle's key with he355_ntt_inverse under prime 0: L in {L_top, 1};
* rgsw_from_bfv == its composition, per slot ciphertext: row f is he355_bfv_transform_to_ntt of it, row E + f he355_bfv_transform_to_ntt of
  he355_bfv_external_product(L, key_bits, 1, 1, it, .., key, 0, 1, ..).  Uniform "ciphertexts" and a uniform "key" (the identity is
  arithmetic): L in {L_top, 1}, (digit_bits, key_bits) in {(20, 20), (20, 4), (45, 20), (63, 63)}, (n, n_sel) in {(1, 1), (2, 3)}, unit strides
  and the child-major strides of an expansion (d_ct at a child behind the first ones); on the N >= 2048 chains n n_sel E 2 L = 62, 64 and 66
  (the column pass runs from 256 blocks = 64 on, the streaming route below); on the 2048 chain at L = 1, key_bits = 4 (2 E_key = 30 rows, below
  the 256-term run of the 60-bit prime) 150 slot ciphertexts, two passes of 136 through the pool block, the last one ragged (the threshold
  and the two-pass cases also assert he355_bfv_route_stats: which cut ran, in how many passes); on n4096_d3 at L = 3, key_bits = 1 one result
  sums 2 E_key = 280 terms, above the run (a fold inside one result); sentinels, operands read back; once behind an unsynchronised he355_add; a second identical call makes no raw allocation;
* meaning, real keys, n4096_d3 at L = 3, digit_bits = key_bits = 20: selectors (0, 1, t - 1) in one query, selector_encrypt -> bfv_expand ->
  rgsw_from_bfv -> external_product on Enc(mu), mu full-range, decrypts to lift(m) mu mod t by Python integers; budgets printed and positive;
* end to end, ONE ciphertext per query, n4096_d3, L = 3 throughout, the 8 x 8 database and the two queries of test_gpu_bfv_external_product.py:
  he355_encrypt of the first dimension's plaintext (2^(-d) mod t at the wanted index) plus selector_encrypt of the eight one-hot column
  selectors at first_slot = 8; v = 20 gives E = 7, count = 8 + 8 * 7 = 64, d = 6; bfv_expand(64), children 0..7 through transform_to_ntt, the
  scan and transform_from_ntt, children 8..63 through rgsw_from_bfv with a key from rgsw_encrypt_secret, external_product with inner = 8 and
  one selector row per query, mod_switch to L = 1, one decrypt gives db[i][j]; the budget is positive after every stage (printed).  The margin
  is bounded without a run: k = 1 rows at most 2^20 * 2^17.3 * 14 * 4096 ~ 2^53; the selection over 8 * 14 rows of 4096 coefficients at most
  ~ 2^92; times t ~ 2^112 against 2^139: about 27 bits in the worst case; measured 54 bits after the external product and 33 in the reply
  (profiles/bfv_selectors.txt).  (Not run at L = 2, v = 20: the same bound does not guarantee a positive budget there.)
* refusals: a CKKS context, a bad L, a bad digit_bits / key_bits, n_sel == 0, count outside 1..N, first_slot + n_sel E > count, every overlap, a
  missing public or secret key (the message says which) -- the code, a message, the output sentinel-clean; n == 0 touches nothing."""
import ctypes as C

import numpy as np
import pytest

import bfv_gadget_ref as gad
import bfv_selector_ref as ref
from bfv_gpu_helpers import SENT, At, be, edged, expand_keys, inner_of, pair, rand_cts, refused, same_allocs, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
CHAINS = ["n1024", N2048, "n4096_d3"]
IDS = ["n1024", "n2048", "n4096_d3"]


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_selector_encrypt_equals_the_definition(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    rng = np.random.default_rng(92)
    t, Lt, n, seed, first = o.t, g.L, 2, 111, 9
    zero = g.alloc(n * 2 * Lt * N)
    g.encrypt_zero(n, seed, first, zero)
    z = zero.download((n, 2, Lt, N))
    fixed = [0, 1, t - 1, t // 2, (t + 1) // 2]
    case = 0
    for L in sorted({Lt, 1}):
        for v in (20, 63):
            E = g.bfv_gadget_count(L, v)[0]
            for n_sel in (1, 3):
                for first_slot in (0, 5):
                    for count in sorted({first_slot + n_sel * E, N}):
                        what = (L, v, n_sel, first_slot, count)
                        sel = rng.integers(0, t, (n, n_sel), dtype=np.uint64)  # full-range, then 0, 1, t - 1, ... in turn over the cases
                        sel[0, 0] = fixed[case % len(fixed)]
                        sel[1, n_sel - 1] = fixed[(case + 1) % 3]
                        case += 1
                        ds = g.to_device(sel)
                        want = ref.np_pack(z[:, :, :L], sel, o.moduli, t, v, first_slot, count)
                        buf = sentinelled(g, n * 2 * L * N, N)
                        g.bfv_selector_encrypt(L, v, n, n_sel, first_slot, count, ds, seed, first, At(buf, N))
                        got = inner_of(buf, N, what).reshape(n, 2, L, N)
                        assert np.array_equal(got, want), what
                        assert np.array_equal(ds.download((n, n_sel)), sel), (what, "selectors")
                        if count == N and n_sel == 3 and first_slot == 5:  # a second identical call: the pool block and the client arena are there
                            g.sync()
                            a = g.alloc_stats()
                            g.bfv_selector_encrypt(L, v, n, n_sel, first_slot, count, ds, seed, first, At(buf, N))
                            g.sync()
                            assert same_allocs(a, g.alloc_stats()), what
                            assert np.array_equal(inner_of(buf, N, what).reshape(n, 2, L, N), want), (what, "again")
                        ds.free()
                        buf.free()
    assert case >= 32
    g.close()


def secret_mod_t(be, g, o, sk, N):
    """the secret key's coefficients mod t: prime 0's residue of the oracle's NTT-form key through he355_ntt_inverse, then 0, 1, q_0 - 1 -> 0, 1, t - 1"""
    s = g.to_device(np.ascontiguousarray(np.asarray(sk, dtype=np.uint64).reshape(-1, N)[0]))
    pm = (C.c_uint8 * 1)(0)
    assert be.lib().he355_ntt_inverse(g.h, s.ptr, 1, pm, 1) == 0
    c = s.download()
    s.free()
    q0 = np.uint64(o.moduli[0])
    assert set(np.unique(c).tolist()) == {0, 1, int(q0) - 1}
    return np.where(c == q0 - np.uint64(1), np.uint64(o.t - 1), c)


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_rgsw_encrypt_secret_equals_the_definition(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    dm = g.to_device(secret_mod_t(be, g, o, sk, N))
    seed, first = 113, 4
    for L in sorted({g.L, 1}):
        for kv in (20, 4):
            rows = 2 * g.bfv_gadget_count(L, kv)[0]
            words = rows * 2 * L * N
            want = g.alloc(words)
            g.bfv_rgsw_encrypt(L, kv, 1, dm, seed, first, want)
            buf = sentinelled(g, words, N)
            g.bfv_rgsw_encrypt_secret(L, kv, seed, first, At(buf, N))
            assert np.array_equal(inner_of(buf, N, (L, kv)), want.download()), (L, kv)
            g.sync()
            a = g.alloc_stats()
            g.bfv_rgsw_encrypt_secret(L, kv, seed, first, At(buf, N))
            g.sync()
            assert same_allocs(a, g.alloc_stats()), (L, kv)
            assert np.array_equal(inner_of(buf, N, (L, kv)), want.download()), (L, kv, "again")
            want.free()
            buf.free()
    g.close()


def composition(g, L, kv, x, order, key, E, N):
    """the definition, per slot ciphertext c (x[order[c]] on the host): row (k = 0) is transform_to_ntt of it, row (k = 1) transform_to_ntt of
    external_product(L, key_bits, 1, 1, it, .., key, 0, 1, ..); laid out by the row rule -> [C / E][2E][2][L][N]"""
    per = 2 * L * N
    C_ = len(order)
    k0, k1 = np.empty((C_, 2, L, N), dtype=np.uint64), np.empty((C_, 2, L, N), dtype=np.uint64)
    one, res = g.alloc(per), g.alloc(per)
    for c, at in enumerate(order):
        one.upload(x[at])
        g.bfv_external_product(L, kv, 1, 1, one, 1, 1, key, 0, 1, res)
        g.bfv_transform_to_ntt(L, 2, 1, res, res)
        g.bfv_transform_to_ntt(L, 2, 1, one, one)
        k0[c], k1[c] = one.download((2, L, N)), res.download((2, L, N))
    one.free()
    res.free()
    return ref.np_rows(k0, k1, E)


def from_bfv_case(g, o, rng, L, v, kv, n, n_sel, child_major, N, what, producer=False, twice=False, routed=None):
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    per = 2 * L * N
    S = n_sel * E  # slot ciphertexts per query
    key = g.alloc(rows * per)
    g.fill_uniform(key, rows * 2 * L, list(range(L)), 2000 + 16 * n + n_sel + v)
    key_before = key.download()
    lead = 2 if child_major else 0  # children before first_slot: d_ct points behind them
    x = edged(o, rng, (lead + S) * n, L)
    if child_major:
        sr, sk_, order = 1, n, [(lead + s) * n + r for r in range(n) for s in range(S)]
    else:
        sr, sk_, order = S, 1, list(range(n * S))
    if producer:  # x = a + b is still being written when the call is queued
        b = rand_cts(o, rng, len(x), L)
        a = np.empty_like(x)
        for i, q in enumerate(o.moduli[:L]):
            q = np.uint64(q)
            a[:, :, i] = np.where(x[:, :, i] >= b[:, :, i], x[:, :, i] - b[:, :, i], x[:, :, i] + (q - b[:, :, i]))
        da, db, dx = g.to_device(a), g.to_device(b), g.to_device(np.zeros_like(x))
    else:
        dx = g.to_device(x)
    words = n * n_sel * 2 * E * per
    buf = sentinelled(g, words, N)
    if producer:
        g.sync()
        g.add(L, 2, len(x), da, db, type(g).pairwise(), dx)
    g.bfv_route_stats(reset=True)
    g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, At(dx, lead * n * per), sr, sk_, key, At(buf, N))
    if routed is not None:  # both cuts give the same bits: the counters of he355_bfv_route_stats say which one ran, and in how many passes
        got_routes = {k: c for k, c in g.bfv_route_stats().items() if c}
        assert got_routes == routed, (what, got_routes)
    got = inner_of(buf, N, what).reshape(n * n_sel, 2 * E, 2, L, N)
    assert np.array_equal(dx.download(x.shape), x), (what, "ciphertexts")
    assert np.array_equal(key.download(), key_before), (what, "key")
    want = composition(g, L, kv, x, order, key, E, N)
    assert np.array_equal(got, want), what
    if twice:  # a second identical call makes no raw allocation
        g.sync()
        first = g.alloc_stats()
        g.bfv_route_stats(reset=True)
        g.bfv_rgsw_from_bfv(L, v, kv, n, n_sel, At(dx, lead * n * per), sr, sk_, key, At(buf, N))
        g.sync()
        assert same_allocs(first, g.alloc_stats()), what
        if routed is not None:
            assert {k: c for k, c in g.bfv_route_stats().items() if c} == routed, (what, "again")
        assert np.array_equal(inner_of(buf, N, what).reshape(got.shape), want), (what, "again")
    for d in (key, dx, buf):
        d.free()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_rgsw_from_bfv_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(93)
    for L in sorted({g.L, 1}):
        for v, kv in ((20, 20), (20, 4), (45, 20), (63, 63)):
            from_bfv_case(g, o, rng, L, v, kv, 1, 1, False, N, (L, v, kv, 1, 1))
            from_bfv_case(g, o, rng, L, v, kv, 2, 3, False, N, (L, v, kv, 2, 3))
            from_bfv_case(g, o, rng, L, v, kv, 2, 3, True, N, (L, v, kv, 2, 3, "child-major"))
    from_bfv_case(g, o, rng, g.L, 20, 20, 2, 3, True, N, "behind an unsynchronised add", producer=True, twice=True)
    g.close()


@pytest.mark.parametrize("chain", CHAINS[1:], ids=IDS[1:])
def test_rgsw_from_bfv_column_pass_threshold(be, oracle, chain):
    """N >= 2048: the column pass runs from 256 blocks on, n n_sel E 2 L 4 >= 256; one short of it, at it, above it (L = 1, one digit per prime)"""
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(94)
    L, v = 1, 63
    E = g.bfv_gadget_count(L, v)[0]
    assert E == 1
    for n, n_sel in ((1, 31), (2, 16), (3, 11)):
        assert n * n_sel * E * 2 * L == {31: 62, 32: 64, 33: 66}[n * n_sel]
        routed = {"own_cols" if n * n_sel * E * 2 * L >= 64 else "own_stream": 1, "passes": 1}
        from_bfv_case(g, o, rng, L, v, 20, n, n_sel, n == 2, N, (n, n_sel), routed=routed)
    g.close()


def test_rgsw_from_bfv_two_passes_the_last_one_ragged(be, oracle):
    g, o, N, *_ = pair(be, oracle, N2048)
    L, v, kv, n, n_sel = 1, 20, 4, 2, 25
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    assert rows == 30 and o.moduli[0].bit_length() == 60
    run = (2 ** 128 - 1) // (o.moduli[0] - 1) ** 2
    assert run == 256 > rows
    per_pass, slots = 4096 // rows, n * n_sel * E
    assert per_pass < slots < 2 * per_pass and slots % per_pass  # two passes through the pool block, the last one ragged
    # the cut is decided once per call, from the first pass: 136 slot ciphertexts are far above the column pass's threshold
    from_bfv_case(g, o, np.random.default_rng(95), L, v, kv, n, n_sel, True, N, "two passes", twice=True, routed={"own_cols": 2, "passes": 2})
    g.close()


def test_rgsw_from_bfv_more_terms_than_a_run(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    L, v, kv = g.L, 63, 1
    rows = 2 * g.bfv_gadget_count(L, kv)[0]
    run = (2 ** 128 - 1) // (o.moduli[0] - 1) ** 2
    assert rows == 280 > run == 256  # the sums of one result are folded once on the way
    from_bfv_case(g, o, np.random.default_rng(96), L, v, kv, 1, 1, False, N, "a fold inside one result")
    g.close()


def test_meaning_with_real_keys(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(97)
    L, v, kv, t = g.L, 20, 20, o.t
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    per = 2 * L * N
    ms = [0, 1, t - 1]
    n_sel = len(ms)
    count = n_sel * E
    expand_keys(g, o, sk, count, 170)
    query, kids, key = g.alloc(per), g.alloc(count * per), g.alloc(rows * per)
    g.bfv_selector_encrypt(L, v, 1, n_sel, 0, count, g.to_device(np.array([ms], dtype=np.uint64)), 121, 0, query)
    g.bfv_expand(L, 1, query, count, kids)
    g.bfv_rgsw_encrypt_secret(L, kv, 122, 0, key)
    rg = g.alloc(n_sel * 2 * E * per)
    g.bfv_rgsw_from_bfv(L, v, kv, 1, n_sel, kids, 1, 1, key, rg)
    mu = rng.integers(0, t, (n_sel, N), dtype=np.uint64)
    mu[0, :4] = [0, 1, t - 1, t // 2]
    mu[2, :4] = [0, 1, t - 1, t // 2]
    ct, out, dec = g.alloc(n_sel * per), g.alloc(n_sel * per), g.alloc(n_sel * N)
    g.encrypt(n_sel, g.to_device(mu), 123, 0, ct)
    g.bfv_external_product(L, v, n_sel, 1, ct, 1, 1, rg, 1, 1, out)
    fresh, budget = g.bfv_noise_budget(L, 2, n_sel, ct), g.bfv_noise_budget(L, 2, n_sel, out)
    print(f"packed selectors (L = {L}, v = key_bits = {v}, d = {ref.depth(count)}): noise budget {fresh.min()} fresh, {list(budget)} after the external product with the expanded RGSW(0, 1, t - 1)")
    assert (budget > 0).all(), budget
    g.decrypt(L, 2, n_sel, out, dec)
    got = dec.download((n_sel, N))
    for r, m in enumerate(ms):
        want = np.array([gad.lift(m, t) * int(c) % t for c in mu[r]], dtype=np.uint64)
        assert np.array_equal(got[r], want), m
    g.close()


def test_end_to_end_one_ciphertext_per_query(be, oracle):
    n1 = n2 = 8
    n, idx = 2, [(5, 2), (0, 7)]
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    L, t, v, kv = g.L, o.t, 20, 20
    assert L == 3
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    count = n1 + n2 * E
    d = ref.depth(count)
    assert (E, count, d) == (7, 64, 6)
    expand_keys(g, o, sk, count, 180)
    rng = np.random.default_rng(76)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)  # the database of test_gpu_bfv_external_product.py
    db[5, 2, :4] = [0, 1, t - 1, t // 2]
    qp = np.zeros((n, N), dtype=np.uint64)
    sel = np.zeros((n, n2), dtype=np.uint64)  # the one-hot column selectors
    for r, (i, j) in enumerate(idx):
        qp[r, i] = pow(1 << d, -1, t)
        sel[r, j] = 1
    per = 2 * L * N
    pw = be.Context.pairwise()
    budgets = {}
    # the client: ONE ciphertext per query, and the key once
    first_dim, packed, query = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    g.encrypt(n, g.to_device(qp), 94, 0, first_dim)
    budgets["fresh"] = g.bfv_noise_budget(L, 2, n, first_dim)
    g.bfv_selector_encrypt(L, v, n, n2, n1, count, g.to_device(sel), 95, 0, packed)
    g.add(L, 2, n, first_dim, packed, pw, query)
    key = g.alloc(rows * per)
    g.bfv_rgsw_encrypt_secret(L, kv, 96, 0, key)
    # the server
    kids = g.alloc(count * n * per)
    g.bfv_expand(L, n, query, count, kids)                                                   # child k of query r at k n + r
    budgets["expand, children 0..7"] = g.bfv_noise_budget(L, 2, n1 * n, kids)
    g.bfv_transform_to_ntt(L, 2, n1 * n, kids, kids)                                         # children 0..7
    dbn = g.alloc(n1 * n2 * L * N)
    g.bfv_plain_to_ntt(L, n1 * n2, g.to_device(db.reshape(n1 * n2, N)), dbn)
    res1 = g.alloc(n * n2 * per)
    g.bfv_multiply_plain_accumulate(L, 2, n, n2, n1, kids, 1, n, dbn, n2, 1, res1)           # result (r, j) = Enc(db[i_r][j])
    g.bfv_transform_from_ntt(L, 2, n * n2, res1, res1)
    budgets["scan"] = g.bfv_noise_budget(L, 2, n * n2, res1)
    rg = g.alloc(n * n2 * 2 * E * per)
    g.bfv_rgsw_from_bfv(L, v, kv, n, n2, At(kids, n1 * n * per), 1, n, key, rg)              # children 8..63 -> RGSW (r, j)
    one = g.alloc(n * per)
    g.bfv_external_product(L, v, n, n2, res1, n2, 1, rg, n2, 1, one)                         # ONE ciphertext per query
    budgets["external product"] = g.bfv_noise_budget(L, 2, n, one)
    low = g.alloc(n * 2 * N)
    g.bfv_mod_switch(L, 1, 2, n, one, low)
    budgets["reply (L = 1)"] = g.bfv_noise_budget(1, 2, n, low)
    final = g.alloc(n * N)
    g.decrypt(1, 2, n, low, final)                                                           # one decrypt per query
    print(f"two-dimensional retrieval, one query ciphertext of {per * 8} bytes: noise budgets (bits) " + ", ".join(f"{k} {b.min()}..{b.max()}" for k, b in budgets.items()))
    for k, b in budgets.items():
        assert (b > 0).all(), (k, b)
    assert np.array_equal(final.download((n, N)), np.stack([db[i, j] for i, j in idx]))
    g.close()


def test_refusals(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3")  # no keys
    rng = np.random.default_rng(98)
    L, v = g.L, 20
    E = g.bfv_gadget_count(L, v)[0]
    rows, per = 2 * E, 2 * L * N
    x = rand_cts(o, rng, 2 * E, L)
    dx = g.to_device(x)
    sel_h = np.array([[1, 0]], dtype=np.uint64)
    ds = g.to_device(sel_h)
    out = g.to_device(np.full(2 * rows * per, SENT, dtype=np.uint64))  # query ciphertexts, a key or RGSW ciphertexts
    key = g.to_device(np.full(rows * per, SENT, dtype=np.uint64))
    se = lambda L_=L, w=v, n=1, n_sel=2, first=3, count=64, sel=ds, dst=out: g.bfv_selector_encrypt(L_, w, n, n_sel, first, count, sel, 1, 0, dst)
    es = lambda L_=L, w=v, dst=out: g.bfv_rgsw_encrypt_secret(L_, w, 1, 0, dst)
    fb = lambda L_=L, w=v, kw=v, n=1, n_sel=2, ct=dx, sr=1, sk_=1, k=key, dst=out: g.bfv_rgsw_from_bfv(L_, w, kw, n, n_sel, ct, sr, sk_, k, dst)
    for f in (se, es, fb):
        for bad in (dict(L_=0), dict(L_=L + 1), dict(w=0), dict(w=64), dict(w=-1)):
            refused(be, lambda: f(**bad))
    for bad in (dict(kw=0), dict(kw=64), dict(n_sel=0), dict(n=2 ** 31), dict(n=2, sr=2 ** 60), dict(sk_=2 ** 60),
                dict(ct=out), dict(ct=At(out, 2 * rows * per - 1)), dict(dst=At(dx, 2 * E * per - 1)), dict(k=out), dict(dst=At(key, rows * per - 1))):
        refused(be, lambda: fb(**bad))
    for bad in (dict(n_sel=0), dict(count=0), dict(count=N + 1), dict(first=64 - 2 * E + 1), dict(count=2 * E + 2), dict(n=2 ** 31),
                dict(sel=out), dict(sel=At(out, per - 1))):
        refused(be, lambda: se(**bad))
    se(n=0)
    fb(n=0)

    def missing(f, which):
        with pytest.raises(be.HE355Error) as ei:
            f()
        assert ei.value.code == be.E_INVALID_ARGS and which in str(ei.value), ei.value

    missing(se, "public key")            # valid arguments, no public key
    missing(es, "secret key")            # neither key: the secret key is asked for first
    o_sk = o.keygen_secret(21)
    g.set_secret_key(o_sk)
    missing(es, "public key")            # the secret key alone
    assert (out.download() == SENT).all() and (key.download() == SENT).all()
    assert np.array_equal(dx.download(x.shape), x) and np.array_equal(ds.download(sel_h.shape), sel_h)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(2 * per), ck.to_device(np.full(rows * per, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_selector_encrypt(1, v, 1, 1, 0, 8, a, 1, 0, b))
    refused(be, lambda: ck.bfv_rgsw_encrypt_secret(1, v, 1, 0, b))
    refused(be, lambda: ck.bfv_rgsw_from_bfv(1, v, v, 1, 1, a, 1, 1, At(a, per), b))
    assert (b.download() == SENT).all()
    ck.close()
