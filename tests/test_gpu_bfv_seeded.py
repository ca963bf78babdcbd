"""GPU parity of seeded BFV queries and Galois keys (he355_bfv_seeded_encrypt, he355_bfv_seeded_selector_encrypt, he355_bfv_seeded_restore,
he355_keygen_galois_seeded, he355_set_galois_key_seeded) against the definition in numpy and Python integers (tests/bfv_seeded_ref.py),
bit-exact (np.array_equal, no tolerance).  Chains: n1024 (Shoup form, no column pass), n4096_d3 (fold form), (2048, {40, 60, 60}) and
(2048, {42, 38, 45, 44}) -- the smallest shapes that reach both engine forms, the ring without a column pass and a mixed fp64 / u64 layout.

* encrypt / selector_encrypt / restore: n = 33 (the calls do not chunk: they work in place on their output and hold no scratch), plaintexts from
  plains(), L = L_top and L = 1, both restore forms; rows 0, 1, 3, 32 against the reference; outputs in sentinelled buffers with the guards
  intact, operands read back unchanged; first_index split across two calls gives the bits of one call; a second identical call makes no raw
  allocation.  The public seed is BUILT on the CPU (the inverse of splitmix64) so that coefficient 700 of ciphertext 1 takes a second draw
  under prime 0 of every chain -- the chains' primes reject one draw in 2^25 .. 2^46 -- and the test asserts that on the reference side;
* composition: restore(0) of seeded_encrypt == he355_bfv_add_plain on restore(0) of the seeded zero; restore(1) == he355_bfv_transform_to_ntt
  of restore(0); he355_decrypt returns the plaintext; he355_bfv_noise_budget is not below that of he355_encrypt of the same plaintext;
* keys: keygen_galois_seeded's halves equal the reference; a context installed with set_galois_key_seeded and a second one given the same
  (b, a) through he355_set_galois_key apply_galois bit-identically, on uniform inputs and on an encryption, which decrypts to the permuted
  plaintext; he355_keygen_galois(seed) applies bit-identically to the reference key with a_seed = noise_seed = seed set through
  he355_set_galois_key: the split seed changed nothing (the oracle's own keygen_galois draws from another generator and never gave the
  device's bits: tests/test_gpu_client.py holds the device key to the host client's, which stays as it is);
* end to end at n4096_d3: the client makes a seeded packed query (first-dimension one-hot plus selectors, added as c0's); only c0, the seed and
  the seeded expansion keys cross to a second context that holds no secret key (RGSW(s) crosses in full: seeding it is not built); there:
  restore, he355_bfv_expand, the scan and the selection of test_gpu_bfv_selectors.py; the reply decrypts to db[i][j]; the query is exactly half
  of the unseeded one's words plus 8 bytes of seed;
* large ring: n32768_d3, n = 2, restore in both forms against the reference, once;
* refusals with a device behind the context, the missing secret key among them; n == 0 touches nothing."""
import numpy as np
import pytest

import bfv_seeded_ref as ref
import bfv_selector_ref as selr
from bfv_gpu_helpers import SENT, At, be, inner_of, pair, plains, rand_cts, refused, same_allocs, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

CHAINS = ["n1024", "n4096_d3", (2048, [40, 60, 60], 20), (2048, [42, 38, 45, 44], 20), "n16384_shoup"]  # the last: the Shoup build at LOGN1 = 4
IDS = ["n1024", "n4096_d3", "n2048_40_60_60", "n2048_42_38_45_44", "n16384_shoup"]
E_SEED = 0x5EC4E75EED
FIRST = 1000
ROWS = (0, 1, 3, 32)
n = 33


def public_seed(o):
    """a seed under which coefficient 700 of seeded ciphertext FIRST + 1 takes a second draw under prime 0"""
    return ref.seed_with_second_draw(ref.a_stream(FIRST + 1, 0), 700, o.moduli[0])


def permuted(m, elt, t, N):
    """m(X^elt) mod t"""
    out = np.zeros(N, dtype=np.uint64)
    for e in range(N):
        at = e * elt % (2 * N)
        out[at % N] = m[e] if at < N else (t - int(m[e])) % t
    return out


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_encrypt_and_restore_equal_the_reference(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    rng = np.random.default_rng(301)
    A = public_seed(o)
    assert 700 in ref.second_draws(A, ref.a_stream(FIRST + 1, 0), N, o.moduli[0]), "an operand of this test takes a second draw"
    m = plains(o, rng, n, N)
    dp = g.to_device(m)
    for L in sorted({g.L, 1}, reverse=True):
        per = L * N
        buf = sentinelled(g, n * per, N)
        g.bfv_seeded_encrypt(L, n, dp, A, E_SEED, FIRST, At(buf, N))
        c0 = inner_of(buf, N, ("encrypt", L)).reshape(n, L, N)
        assert np.array_equal(dp.download((n, N)), m), "plaintexts"
        for r in ROWS:
            assert np.array_equal(c0[r], ref.encrypt(o, sk, L, m[r:r + 1], A, E_SEED, FIRST + r)[0]), (L, r)
        # a second identical call makes no raw allocation; first_index split across two calls gives the same bits
        g.sync()
        a = g.alloc_stats()
        g.bfv_seeded_encrypt(L, n, dp, A, E_SEED, FIRST, At(buf, N))
        g.sync()
        assert same_allocs(a, g.alloc_stats()), L
        two = sentinelled(g, n * per, N)
        g.bfv_seeded_encrypt(L, 20, dp, A, E_SEED, FIRST, At(two, N))
        g.bfv_seeded_encrypt(L, n - 20, At(dp, 20 * N), A, E_SEED, FIRST + 20, At(two, N + 20 * per))
        assert np.array_equal(inner_of(two, N, ("split", L)).reshape(n, L, N), c0), L
        # NULL plaintexts: the seeded zero
        zb = sentinelled(g, 2 * per, N)
        g.bfv_seeded_encrypt(L, 2, None, A, E_SEED, FIRST, At(zb, N))
        z = inner_of(zb, N, ("zero", L)).reshape(2, L, N)
        assert np.array_equal(z[1], ref.seeded_zero(o, sk, L, A, E_SEED, FIRST + 1)[0]), L
        # restore, both forms
        dc = g.to_device(c0)
        for form in (0, 1):
            out = sentinelled(g, n * 2 * per, N)
            g.bfv_seeded_restore(L, form, n, dc, A, FIRST, At(out, N))
            got = inner_of(out, N, ("restore", L, form)).reshape(n, 2, L, N)
            assert np.array_equal(dc.download((n, L, N)), c0), "c0"
            for r in ROWS:
                assert np.array_equal(got[r], ref.restore(o, L, form, c0[r:r + 1], A, FIRST + r)[0]), (L, form, r)
            g.sync()
            a = g.alloc_stats()
            g.bfv_seeded_restore(L, form, n, dc, A, FIRST, At(out, N))
            g.sync()
            assert same_allocs(a, g.alloc_stats()), (L, form)
            two = sentinelled(g, n * 2 * per, N)
            g.bfv_seeded_restore(L, form, 13, dc, A, FIRST, At(two, N))
            g.bfv_seeded_restore(L, form, n - 13, At(dc, 13 * per), A, FIRST + 13, At(two, N + 13 * 2 * per))
            assert np.array_equal(inner_of(two, N, ("restore split", L, form)).reshape(n, 2, L, N), got), (L, form)
            out.free()
            two.free()
        for d in (buf, zb, dc):
            d.free()
    g.close()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_selector_encrypt_equals_the_reference(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    rng = np.random.default_rng(302)
    A, t, v, n_sel, first_slot = public_seed(o), o.t, 20, 3, 5
    for L in sorted({g.L, 1}, reverse=True):
        E = g.bfv_gadget_count(L, v)[0]
        for count in sorted({first_slot + n_sel * E, N}):
            sel = rng.integers(0, t, (n, n_sel), dtype=np.uint64)
            sel[0] = [0, 1, t - 1]
            sel[32, 0] = t // 2
            ds = g.to_device(sel)
            buf = sentinelled(g, n * L * N, N)
            g.bfv_seeded_selector_encrypt(L, v, n, n_sel, first_slot, count, ds, A, E_SEED, FIRST, At(buf, N))
            got = inner_of(buf, N, (L, count)).reshape(n, L, N)
            assert np.array_equal(ds.download((n, n_sel)), sel), "selectors"
            for r in ROWS:
                assert np.array_equal(got[r], ref.selector_c0(o, sk, L, v, sel[r:r + 1], first_slot, count, A, E_SEED, FIRST + r)[0]), (L, count, r)
            two = sentinelled(g, n * L * N, N)
            g.bfv_seeded_selector_encrypt(L, v, 32, n_sel, first_slot, count, ds, A, E_SEED, FIRST, At(two, N))
            g.bfv_seeded_selector_encrypt(L, v, 1, n_sel, first_slot, count, At(ds, 32 * n_sel), A, E_SEED, FIRST + 32, At(two, N + 32 * L * N))
            assert np.array_equal(inner_of(two, N, ("split", L, count)).reshape(n, L, N), got), (L, count)
            for d in (ds, buf, two):
                d.free()
    g.close()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_composition_with_the_existing_calls(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    rng = np.random.default_rng(303)
    A, k = public_seed(o), 4
    m = plains(o, rng, k, N)
    dp = g.to_device(m)
    pw = be.Context.pairwise()
    for L in sorted({g.L, 1}, reverse=True):
        per = 2 * L * N
        c0, z0 = g.alloc(k * L * N), g.alloc(k * L * N)
        g.bfv_seeded_encrypt(L, k, dp, A, E_SEED, FIRST, c0)
        g.bfv_seeded_encrypt(L, k, None, A, E_SEED, FIRST, z0)
        ct, zero, ntt, want = g.alloc(k * per), g.alloc(k * per), g.alloc(k * per), g.alloc(k * per)
        g.bfv_seeded_restore(L, 0, k, c0, A, FIRST, ct)
        g.bfv_seeded_restore(L, 0, k, z0, A, FIRST, zero)
        g.bfv_add_plain(L, 2, k, zero, dp, pw, want)
        assert np.array_equal(ct.download(), want.download()), (L, "add_plain on the seeded zero")
        g.bfv_seeded_restore(L, 1, k, c0, A, FIRST, ntt)
        g.bfv_transform_to_ntt(L, 2, k, ct, want)
        assert np.array_equal(ntt.download(), want.download()), (L, "transform_to_ntt of the other form")
        dec = g.alloc(k * N)
        g.decrypt(L, 2, k, ct, dec)
        assert np.array_equal(dec.download((k, N)), m), L
        seeded = g.bfv_noise_budget(L, 2, k, ct)
        if L == g.L:  # he355_encrypt makes top-level ciphertexts
            g.encrypt(k, dp, 77, 0, want)
            public = g.bfv_noise_budget(L, 2, k, want)
            print(f"noise budget at L = {L}: seeded {list(seeded)}, public-key {list(public)}")
            assert (seeded >= public).all(), (seeded, public)
        assert (seeded > 0).all()
        for d in (c0, z0, ct, zero, ntt, want, dec):
            d.free()
    g.close()


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_seeded_galois_keys(be, oracle, chain):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    g2 = pair(be, oracle, chain)[0]  # the server: no secret key
    rng = np.random.default_rng(304)
    A, Lt, K, t = public_seed(o), g.L, g.K, o.t
    elt = N // 2 + 1
    buf = sentinelled(g, Lt * K * N, N)
    g.keygen_galois_seeded(elt, A, E_SEED, At(buf, N))
    b = inner_of(buf, N, "b halves").reshape(Lt, K, N)
    b_ref, a_ref = ref.galois_key(o, sk, elt, A, E_SEED)
    assert np.array_equal(b, b_ref)
    g.sync()
    st = g.alloc_stats()
    g.keygen_galois_seeded(elt, A, E_SEED, At(buf, N))
    g.sync()
    assert same_allocs(st, g.alloc_stats())
    g.set_galois_key_seeded(elt, b, A)
    g2.set_galois_key(elt, ref.full_key(b_ref, a_ref))
    k = 3
    m = plains(o, rng, 1, N)
    x = rand_cts(o, rng, k, Lt)
    x[0] = ref.restore(o, Lt, 0, ref.encrypt(o, sk, Lt, m, A, E_SEED, 7), A, 7)[0]
    outs = []
    for c in (g, g2):
        dx, out = c.to_device(x), c.alloc(k * 2 * Lt * N)
        c.apply_galois(Lt, k, dx, elt, out)
        outs.append(out.download((k, 2, Lt, N)))
    assert np.array_equal(outs[0], outs[1]), "the seeded key is the full key"
    assert np.array_equal(outs[0][1], o.apply_galois(x[1], elt, ref.full_key(b_ref, a_ref))), "and the oracle's result under it"
    dec = g.alloc(N)
    g.decrypt(Lt, 2, 1, g.to_device(outs[0][0]), dec)
    assert np.array_equal(dec.download(), permuted(m[0], elt, t, N))
    # the split seed changed nothing: he355_keygen_galois(seed) is the key of a_seed = noise_seed = seed
    seed, elt2 = 0xBEEF, 3
    g.keygen_galois(elt2, seed)
    g2.set_galois_key(elt2, ref.full_key(*ref.galois_key(o, sk, elt2, seed, seed)))
    outs = []
    for c in (g, g2):
        dx, out = c.to_device(x), c.alloc(k * 2 * Lt * N)
        c.apply_galois(Lt, k, dx, elt2, out)
        outs.append(out.download((k, 2, Lt, N)))
    assert np.array_equal(outs[0], outs[1]), "he355_keygen_galois draws a and e from its one seed as before"
    g.close()
    g2.close()


def test_end_to_end_seeded_query(be, oracle):
    n1 = n2 = 8
    q, idx = 2, [(5, 2), (0, 7)]
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)   # the client
    s = pair(be, oracle, "n4096_d3")[0]                          # the server: no key of the client's
    L, t, v, kv = g.L, o.t, 20, 20
    E, rows = g.bfv_gadget_count(L, v)[0], 2 * g.bfv_gadget_count(L, kv)[0]
    count = n1 + n2 * E
    d = selr.depth(count)
    assert (L, E, count, d) == (3, 7, 64, 6)
    A, IA, IB = public_seed(o), 0, 1 << 20  # the two index ranges are the protocol's constants
    rng = np.random.default_rng(76)
    db = rng.integers(0, t, (n1, n2, N), dtype=np.uint64)
    db[5, 2, :4] = [0, 1, t - 1, t // 2]
    qp = np.zeros((q, N), dtype=np.uint64)
    sel = np.zeros((q, n2), dtype=np.uint64)
    for r, (i, j) in enumerate(idx):
        qp[r, i] = pow(1 << d, -1, t)
        sel[r, j] = 1
    per = 2 * L * N
    pw = be.Context.pairwise()
    # the client: ONE c0 per query, the b halves of the expansion keys, and RGSW(s) (in full: seeding it is not built)
    c0a, c0b, c0q = g.alloc(q * L * N), g.alloc(q * L * N), g.alloc(q * L * N)
    g.bfv_seeded_encrypt(L, q, g.to_device(qp), A, E_SEED, IA, c0a)
    g.bfv_seeded_selector_encrypt(L, v, q, n2, n1, count, g.to_device(sel), A, E_SEED, IB, c0b)
    g.add(L, 1, q, c0a, c0b, pw, c0q)
    wire_query = c0q.download()
    halves = {}
    kb = g.alloc(L * g.K * N)
    for e in g.bfv_expand_galois_elts(count):
        g.keygen_galois_seeded(e, A, E_SEED, kb)
        halves[e] = kb.download((L, g.K, N))
    key_c = g.alloc(rows * per)
    g.bfv_rgsw_encrypt_secret(L, kv, 96, 0, key_c)
    wire_rgsw = key_c.download()
    assert wire_query.nbytes + 8 == q * per * 8 // 2 + 8, "half of the unseeded query's words, plus 8 bytes of seed"
    assert all(h.nbytes * 2 == L * 2 * g.K * N * 8 for h in halves.values()), "and half of every expansion key"
    # the server
    for e, h in halves.items():
        s.set_galois_key_seeded(e, h, A)
    qa, qb, query = s.alloc(q * per), s.alloc(q * per), s.alloc(q * per)
    s.bfv_seeded_restore(L, 0, q, s.to_device(wire_query), A, IA, qa)
    s.bfv_seeded_restore(L, 0, q, s.to_device(np.zeros(q * L * N, dtype=np.uint64)), A, IB, qb)
    s.add(L, 2, q, qa, qb, pw, query)
    key = s.to_device(wire_rgsw)
    kids = s.alloc(count * q * per)
    s.bfv_expand(L, q, query, count, kids)
    s.bfv_transform_to_ntt(L, 2, n1 * q, kids, kids)
    dbn = s.alloc(n1 * n2 * L * N)
    s.bfv_plain_to_ntt(L, n1 * n2, s.to_device(db.reshape(n1 * n2, N)), dbn)
    res1 = s.alloc(q * n2 * per)
    s.bfv_multiply_plain_accumulate(L, 2, q, n2, n1, kids, 1, q, dbn, n2, 1, res1)
    s.bfv_transform_from_ntt(L, 2, q * n2, res1, res1)
    rg = s.alloc(q * n2 * 2 * E * per)
    s.bfv_rgsw_from_bfv(L, v, kv, q, n2, At(kids, n1 * q * per), 1, q, key, rg)
    one = s.alloc(q * per)
    s.bfv_external_product(L, v, q, n2, res1, n2, 1, rg, n2, 1, one)
    low = s.alloc(q * 2 * N)
    s.bfv_mod_switch(L, 1, 2, q, one, low)
    reply = low.download()
    # the client
    dr = g.to_device(reply)
    budget = g.bfv_noise_budget(1, 2, q, dr)
    print(f"seeded two-dimensional retrieval: query {wire_query.nbytes // q} + 8 bytes against {per * 8} unseeded; reply budget {list(budget)} bits")
    assert (budget > 0).all(), budget
    final = g.alloc(q * N)
    g.decrypt(1, 2, q, dr, final)
    assert np.array_equal(final.download((q, N)), np.stack([db[i, j] for i, j in idx]))
    g.close()
    s.close()


def test_large_ring_restore(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n32768_d3")
    rng = np.random.default_rng(305)
    A, L, k = public_seed(o), g.L, 2
    c0 = np.stack([o.random_poly(rng, L, 1)[0] for _ in range(k)])
    dc = g.to_device(c0)
    for form in (0, 1):
        out = sentinelled(g, k * 2 * L * N, N)
        g.bfv_seeded_restore(L, form, k, dc, A, FIRST, At(out, N))
        got = inner_of(out, N, form).reshape(k, 2, L, N)
        assert np.array_equal(got, ref.restore(o, L, form, c0, A, FIRST)), form
        out.free()
    g.close()


def test_refusals(be, oracle):
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3")  # no keys
    L, v, A = g.L, 20, 11
    E = g.bfv_gadget_count(L, v)[0]
    c0 = g.to_device(np.full(2 * L * N, SENT, dtype=np.uint64))
    out = g.to_device(np.full(2 * 2 * L * N, SENT, dtype=np.uint64))
    kb = g.to_device(np.full(L * g.K * N, SENT, dtype=np.uint64))
    pl_h = np.arange(2 * N, dtype=np.uint64) % np.uint64(o.t)
    pl = g.to_device(pl_h)
    enc = lambda L_=L, k=2, p=pl, a=A, e=E_SEED, first=0, dst=c0: g.bfv_seeded_encrypt(L_, k, p, a, e, first, dst)
    se = lambda L_=L, w=v, k=2, n_sel=2, slot=3, count=64, s=pl, a=A, e=E_SEED, first=0, dst=c0: g.bfv_seeded_selector_encrypt(L_, w, k, n_sel, slot, count, s, a, e, first, dst)
    res = lambda L_=L, form=0, k=2, src=c0, first=0, dst=out: g.bfv_seeded_restore(L_, form, k, src, A, first, dst)
    kg = lambda elt=3, a=A, e=E_SEED: g.keygen_galois_seeded(elt, a, e, kb)
    for f in (enc, se, res):
        for bad in (dict(L_=0), dict(L_=L + 1), dict(first=(1 << 40) - 1), dict(first=2 ** 64 - 1), dict(k=2 ** 31)):
            refused(be, lambda: f(**bad))
    for f in (enc, se, kg):
        refused(be, lambda: f(a=5, e=5))
    for bad in (dict(p=c0), dict(dst=At(pl, 2 * N - 1))):
        refused(be, lambda: enc(**bad))
    for bad in (dict(w=0), dict(w=64), dict(n_sel=0), dict(count=0), dict(count=N + 1), dict(slot=64 - 2 * E + 1), dict(s=c0), dict(dst=At(pl, 3))):
        refused(be, lambda: se(**bad))
    for bad in (dict(form=2), dict(form=-1), dict(dst=c0), dict(src=At(out, 4 * L * N - 1)), dict(dst=At(c0, 2 * L * N - 1))):
        refused(be, lambda: res(**bad))
    for elt in (0, 1, 4, 2 * N, 2 * N + 1):
        refused(be, lambda: kg(elt=elt))
        refused(be, lambda: g.set_galois_key_seeded(elt, np.zeros((L, g.K, N), dtype=np.uint64), A))

    def missing(f):
        with pytest.raises(be.HE355Error) as ei:
            f()
        assert ei.value.code == be.E_INVALID_ARGS and "secret key" in str(ei.value), ei.value

    for f in (enc, se, kg):  # valid arguments, no secret key: refused before the first launch
        missing(f)
    res(k=0)
    res()  # the server's call needs no key
    g.set_secret_key(o.keygen_secret(21))
    enc(k=0)  # with the key there, n == 0 touches nothing
    se(k=0)
    g.sync()
    assert (c0.download() == SENT).all() and (kb.download() == SENT).all() and np.array_equal(pl.download(), pl_h)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.alloc(2 * N), ck.to_device(np.full(4 * N, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_seeded_encrypt(1, 1, a, 1, 2, 0, b))
    refused(be, lambda: ck.bfv_seeded_selector_encrypt(1, v, 1, 1, 0, 8, a, 1, 2, 0, b))
    refused(be, lambda: ck.bfv_seeded_restore(1, 0, 1, a, 1, 0, b))
    refused(be, lambda: ck.keygen_galois_seeded(3, 1, 2, b))
    refused(be, lambda: ck.set_galois_key_seeded(3, np.zeros((ck.L, ck.K, N), dtype=np.uint64), 1))
    assert (b.download() == SENT).all()
    ck.close()
