"""GPU parity of the BFV monomial multiply and the oblivious query expansion (he355_bfv_multiply_monomial, he355_bfv_expand_galois_elts,
he355_bfv_expand), bit-exact (np.array_equal, no tolerance):

* monomial  : out = in X^e against a numpy negacyclic shift AND bit for bit against he355_bfv_multiply_plain with the matching monomial
              plaintext (X^e, or (t - 1) X^(e - N) for e >= N); chains n1024 (Shoup form), n4096_d3 (fold form), (2048, {60, 40, 60});
              L = L_top and 1; sizes 1..3; n = 3; e in {0, 1, 2, 3, 1023, 1024, 1025, N - 1, N, N + 1, 2N - 1}; uniform rows mixed with
              all-0 and all-(q - 1) rows; a sentinel before and after the output, the input read back;
* refusals  : CKKS context, e >= 2N, size 0 / 4, bad L, count 0 / N + 1, a missing Galois key (named in the message), overlaps: the code,
              a message, and the output untouched; n == 0 touches nothing;
* expansion : every child of every query against the definition run in the oracle (oracle.apply_galois, oracle.add / oracle.sub, a numpy
              shift), n1024 at L = 2, n4096_d3 at L = 3 and L = 2, count in {1, 2, 5, 8, 16}, n in {1, 3}, a real encryption and random_poly
              ciphertexts, keys from oracle.keygen_galois; again under set_chunk(2); again behind an unsynchronised he355_add;
* deep tree : (2048, {60, 40, 60}), count = 2048 (d = 11, shifts up to a whole 1024-word row), real keys, a full-range plaintext: all 2048
              children decrypted on the device equal 2^11 m_k mod t, children 0, 1, 5, 1023, 1024, 2047 followed through the oracle;
* general   : n1024, count 8, full-range m: child k decrypts to 8 sum_{i = k mod 8} m_i X^(i - k);
* end to end: n4096_d3, two queries 2^-4 X^idx -> expand -> to_ntt -> multiply_plain_accumulate over a 16 x 2 database -> from_ntt ->
              decrypt gives the database row, also after he355_bfv_mod_switch to L = 2 and L = 1; the noise budget stays positive;
* a second identical he355_bfv_expand makes no raw hipMalloc."""

import numpy as np
import pytest

from bfv_expand_ref import children, expand_levels, np_shift
from bfv_gpu_helpers import ALL, SENT, At, be, edged, expand_keys, keyed, pair, rand_cts, refused, to_level  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)


def test_np_shift_is_the_schoolbook_product():
    q, N = 97, 8
    rng = np.random.default_rng(3)
    a = rng.integers(0, q, (1, N), dtype=np.uint64)
    a[0, 2] = 0
    for e in range(2 * N):
        want = [0] * N
        for i in range(N):
            want[(i + e) % N] = (want[(i + e) % N] + (-1 if ((i + e) // N) & 1 else 1) * int(a[0, i])) % q
        assert np_shift(a, e, [q])[0].tolist() == want, e


def monomial_plain(t, N, e):
    m = np.zeros((1, N), dtype=np.uint64)
    m[0, e % N] = 1 if e < N else t - 1
    return m


@pytest.mark.parametrize("chain", ["n1024", "n4096_d3", N2048], ids=["n1024", "n4096_d3", "n2048"])
def test_multiply_monomial(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(61)
    n = 3
    ix = be.Context.outer(0, n, 0, 1)  # ciphertext r, the one plaintext
    for L in sorted({g.L, 1}):
        for size in (1, 2, 3):
            per = size * L * N
            x = edged(o, rng, n, L, size)
            dx = g.to_device(x)
            for e in sorted({0, 1, 2, 3, 1023, 1024, 1025, N - 1, N, N + 1, 2 * N - 1}):
                buf = g.to_device(np.full(n * per + 2 * N, SENT, dtype=np.uint64))
                g.bfv_multiply_monomial(L, size, n, dx, e, At(buf, N))
                got = buf.download()
                assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), (L, size, e, "sentinel")
                got = got[N:-N].reshape(n, size, L, N)
                assert np.array_equal(got, np_shift(x, e, o.moduli)), (L, size, e, "numpy shift")
                ref = g.alloc(n * per)
                g.bfv_multiply_plain(L, size, n, dx, g.to_device(monomial_plain(o.t, N, e)), ix, ref)
                assert np.array_equal(got, ref.download((n, size, L, N))), (L, size, e, "he355_bfv_multiply_plain")
                buf.free()
                ref.free()
            assert np.array_equal(dx.download((n, size, L, N)), x), (L, size, "input")
    g.close()


def test_refusals(be, oracle):
    g, o, N, sk, _ = pair(be, oracle, "n4096_d3", keys=True)
    rng = np.random.default_rng(62)
    L = g.L
    per = 2 * L * N
    x = rand_cts(o, rng, 2, L)
    dx = g.to_device(x)
    out = g.to_device(np.full(8 * per, SENT, dtype=np.uint64))
    mono = lambda L_=L, size=2, n=2, src=dx, e=1, dst=out: g.bfv_multiply_monomial(L_, size, n, src, e, dst)
    refused(be, lambda: mono(e=2 * N))
    refused(be, lambda: mono(e=2 ** 32 - 1))
    refused(be, lambda: mono(size=0))
    refused(be, lambda: mono(size=4))
    refused(be, lambda: mono(L_=0))
    refused(be, lambda: mono(L_=L + 1))
    refused(be, lambda: mono(src=out))
    refused(be, lambda: mono(src=At(out, per)))
    refused(be, lambda: mono(src=At(out, N), n=1))
    mono(n=0)
    elts = g.bfv_expand_galois_elts(4)
    assert elts == [N + 1, N // 2 + 1]
    expand = lambda L_=L, n=2, src=dx, count=4, dst=out: g.bfv_expand(L_, n, src, count, dst)
    with pytest.raises(be.HE355Error) as ei:  # no Galois key at all
        expand()
    assert ei.value.code == be.E_INVALID_ARGS and str(N + 1) in str(ei.value)
    g.set_galois_key(elts[0], o.keygen_galois(sk, elts[0], 70))
    with pytest.raises(be.HE355Error) as ei:  # the second level's key is missing: nothing of the first level may have run
        expand()
    assert ei.value.code == be.E_INVALID_ARGS and str(N // 2 + 1) in str(ei.value)
    assert (out.download() == SENT).all()
    g.set_galois_key(elts[1], o.keygen_galois(sk, elts[1], 71))
    refused(be, lambda: expand(count=0))
    refused(be, lambda: expand(count=N + 1))
    refused(be, lambda: expand(L_=0))
    refused(be, lambda: expand(L_=L + 1))
    refused(be, lambda: expand(src=out))
    refused(be, lambda: expand(src=At(out, 3 * per), n=1))     # the last child's place
    refused(be, lambda: expand(src=At(out, N), n=1, count=1))  # count == 1 is a copy: it may not run over itself either
    expand(n=0)
    assert (out.download() == SENT).all()
    assert np.array_equal(dx.download((2, 2, L, N)), x)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(8 * per), ck.to_device(np.full(8 * per, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_multiply_monomial(ck.L, 2, 1, a, 1, b))
    refused(be, lambda: ck.bfv_expand(ck.L, 1, a, 4, b))
    assert ck.bfv_expand_galois_elts(4) == []
    assert (b.download() == SENT).all()
    ck.close()


# ---- expansion against the definition, run in the oracle -------------------------------------------------------------------------------
_CASES = {}


def expand_case(be, oracle, chain, L):
    """a device / oracle pair with the Galois keys of a depth-4 tree, three queries (a real encryption and two random_poly ciphertexts) at
    level L and their trees in the oracle -- made once, shared by the tests below and left unchanged"""
    if (chain, L) not in _CASES:
        g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
        rng = np.random.default_rng(63 + L)
        gks = expand_keys(g, o, sk, 16, 80)
        assert list(gks) == [N // (1 << j) + 1 for j in range(len(gks))]
        m = rng.integers(0, o.t, N, dtype=np.uint64)
        q = np.stack([to_level(o, o.encrypt(pk, m, 90), L)] + [o.random_poly(rng, L, 2) for _ in range(2)])
        trees = [expand_levels(o, q[r], 4, gks, L) for r in range(3)]
        _CASES[(chain, L)] = (g, o, N, q, trees)
    return _CASES[(chain, L)]


def check_children(got, trees, count, n, what):
    for k in range(count):
        for r in range(n):
            assert np.array_equal(got[k, r], children(trees[r], count)[k]), (what, count, n, "child", k, "query", r)


EXPAND_CASES = [("n1024", 2), ("n4096_d3", 3), ("n4096_d3", 2)]


@pytest.mark.parametrize("chain,L", EXPAND_CASES)
def test_expand_equals_the_definition(be, oracle, chain, L):
    g, o, N, q, trees = expand_case(be, oracle, chain, L)
    per = 2 * L * N
    for n in (1, 3):
        dq = g.to_device(q[:n])
        for count in (1, 2, 5, 8, 16):
            buf = g.to_device(np.full(count * n * per + 2 * N, SENT, dtype=np.uint64))
            g.bfv_expand(L, n, dq, count, At(buf, N))
            got = buf.download()
            assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), (count, n, "sentinel")
            check_children(got[N:-N].reshape(count, n, 2, L, N), trees, count, n, "plain")
            buf.free()
        assert np.array_equal(dq.download((n, 2, L, N)), q[:n])
        dq.free()


@pytest.mark.parametrize("chain,L", EXPAND_CASES)
def test_expand_in_ragged_chunks(be, oracle, chain, L):
    """set_chunk(2), dual stream at its default: the 3, 6, 12, 24 nodes of the level batches are cut into chunks that end mid-node"""
    g, o, N, q, trees = expand_case(be, oracle, chain, L)
    n = 3
    dq = g.to_device(q)
    g.set_chunk(2)
    try:
        for count in (5, 16):
            out = g.alloc(count * n * 2 * L * N)
            g.bfv_expand(L, n, dq, count, out)
            check_children(out.download((count, n, 2, L, N)), trees, count, n, "chunk 2")
            out.free()
    finally:
        g.set_chunk(1024)
    dq.free()


@pytest.mark.parametrize("chain,L", EXPAND_CASES)
def test_expand_behind_an_unsynchronised_producer(be, oracle, chain, L):
    g, o, N, q, trees = expand_case(be, oracle, chain, L)
    n, count = 3, 8
    rng = np.random.default_rng(64)
    y = rand_cts(o, rng, n, L)
    x = np.stack([o.sub(q[r], y[r]) for r in range(n)])  # x + y = q
    dx, dy = g.to_device(x), g.to_device(y)
    a, out = g.to_device(np.zeros_like(q)), g.alloc(count * n * 2 * L * N)
    g.sync()
    g.add(L, 2, n, dx, dy, be.Context.pairwise(), a)
    g.bfv_expand(L, n, a, count, out)
    check_children(out.download((count, n, 2, L, N)), trees, count, n, "producer")
    for b in (dx, dy, a, out):
        b.free()


def test_second_identical_expand_makes_no_raw_allocation(be, oracle):
    g, o, N, q, trees = expand_case(be, oracle, "n4096_d3", 3)
    n, count, L = 3, 16, 3
    dq, out = g.to_device(q), g.alloc(count * n * 2 * L * N)
    g.bfv_expand(L, n, dq, count, out)
    g.sync()
    first = g.alloc_stats()
    g.bfv_expand(L, n, dq, count, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    check_children(out.download((count, n, 2, L, N)), trees, count, n, "second call")
    dq.free()
    out.free()


# ---- what the children decrypt to ---------------------------------------------------------------------------------------------
def test_deep_tree(be, oracle):
    """count = N = 2048: 11 levels, 2047 key switches, the last level's shift a whole 1024-word row; 128 MiB of children"""
    count = 2048
    g, o, N, sk, pk, gks = keyed(be, oracle, N2048, count, 100)
    assert N == count and len(gks) == 11 and min(gks) == 3
    L, t = g.L, o.t
    rng = np.random.default_rng(65)
    m = rng.integers(0, t, N, dtype=np.uint64)
    m[:4] = [0, 1, t - 1, t // 2]
    q = o.encrypt(pk, m, 91)
    dq, out, dec = g.to_device(q), g.alloc(count * 2 * L * N), g.alloc(count * N)
    g.bfv_expand(L, 1, dq, count, out)
    g.decrypt(L, 2, count, out, dec)
    want = np.zeros((count, N), dtype=np.uint64)
    want[:, 0] = (m.astype(object) * 2048 % t).astype(np.uint64)
    assert np.array_equal(dec.download((count, N)), want)
    budget = g.bfv_noise_budget(L, 2, count, out)
    print(f"deep tree: noise budget of the 2048 children {budget.min()}..{budget.max()} bits")
    assert (budget > 0).all()
    for k in (0, 1, 5, 1023, 1024, 2047):  # the 11 steps of child k's path: the node at level j is k mod 2^j
        node = q
        for j in range(11):
            s, e = 1 << j, N // (1 << j) + 1
            gal = o.apply_galois(node, e, gks[e])
            node = np_shift(o.sub(node, gal), 2 * N - s, o.moduli) if k & s else o.add(node, gal)
        assert np.array_equal(out.download_range(k * 2 * L * N, (2, L, N)), node), k
    g.close()


def test_general_plaintext_closed_form(be, oracle):
    count = 8
    g, o, N, sk, pk, gks = keyed(be, oracle, "n1024", count, 120)
    L, t = g.L, o.t
    rng = np.random.default_rng(66)
    m = rng.integers(0, t, N, dtype=np.uint64)
    dq, out, dec = g.to_device(o.encrypt(pk, m, 92)), g.alloc(count * 2 * L * N), g.alloc(count * N)
    g.bfv_expand(L, 1, dq, count, out)
    g.decrypt(L, 2, count, out, dec)
    want = np.zeros((count, N), dtype=np.uint64)
    for k in range(count):  # 8 sum_{i = k mod 8} m_i X^(i - k)
        want[k, 0::8] = (m[k::8].astype(object) * 8 % t).astype(np.uint64)
    assert np.array_equal(dec.download((count, N)), want)
    g.close()


def test_end_to_end_retrieval(be, oracle):
    count, n, cols, idx = 16, 2, 2, (11, 0)
    g, o, N, sk, pk, gks = keyed(be, oracle, "n4096_d3", count, 140)
    L, t = g.L, o.t
    assert L == 3
    rng = np.random.default_rng(67)
    db = rng.integers(0, t, (count, cols, N), dtype=np.uint64)  # full-range plaintexts
    qp = np.zeros((n, N), dtype=np.uint64)
    for r in range(n):
        qp[r, idx[r]] = pow(16, -1, t)
    per = 2 * L * N
    query, kids, ptn, res = g.alloc(n * per), g.alloc(count * n * per), g.alloc(count * cols * L * N), g.alloc(n * cols * per)
    g.encrypt(n, g.to_device(qp), 93, 0, query)
    fresh = g.bfv_noise_budget(L, 2, n, query)
    g.bfv_expand(L, n, query, count, kids)
    after_expand = g.bfv_noise_budget(L, 2, count * n, kids)
    g.bfv_transform_to_ntt(L, 2, count * n, kids, kids)
    g.bfv_plain_to_ntt(L, count * cols, g.to_device(db.reshape(count * cols, N)), ptn)
    g.bfv_multiply_plain_accumulate(L, 2, n, cols, count, kids, 1, n, ptn, cols, 1, res)
    g.bfv_transform_from_ntt(L, 2, n * cols, res, res)
    want = np.stack([db[idx[r], j] for r in range(n) for j in range(cols)])
    budgets = {"fresh": fresh, "expand": after_expand}
    cur = res
    for Lc in (3, 2, 1):
        if Lc < L:
            nxt = g.alloc(n * cols * 2 * Lc * N)
            g.bfv_mod_switch(Lc + 1, Lc, 2, n * cols, cur, nxt)
            cur = nxt
        budgets[f"L{Lc}"] = g.bfv_noise_budget(Lc, 2, n * cols, cur)
        dec = g.alloc(n * cols * N)
        g.decrypt(Lc, 2, n * cols, cur, dec)
        assert np.array_equal(dec.download((n * cols, N)), want), Lc
    print("end to end: noise budgets (bits) " + ", ".join(f"{k} {v.min()}..{v.max()}" for k, v in budgets.items()))
    for k, v in budgets.items():
        assert (v > 0).all(), (k, v)
    g.close()
