"""GPU tests of the hoisted rotations (run with -m gpu on an MI355X): he355_apply_galois_hoisted, he355_rotate_hoisted and
he355_rotate_hoisted_plain_sum against their definition -- the composition of oracle calls in tests/rotate_hoisted_ref.py -- bit for bit
(np.array_equal, no tolerance), and with real keys against he355_rotate's plaintexts.

* contexts: CKKS N = 1024 {50,40,40,50} (one row per polynomial, both engines), 2048 {45,52} (L = 1, one digit), 4096 {60,45,45,60} with the u64
  engine forced, 8192 {60,45,60}, and one case at 16384 {60,45,45,45,60}; BFV N = 1024 {50,40,40,50} and 2048 {60,40,60}, t of 20 bits, both
  ntt_form values; levels L_top and L_top - 1 (the key keeps L_top digits, the call uses L of them);
* elements: steps 1, 3, -2 (g != g^-1), the self-inverse 2N - 1, the identity, one element twice, n_elts = 1; batches n = 1, 3, and 5 under
  set_chunk(2) (three chunks, the slab reused, a ragged last chunk);
* operands: uniform, all q_i - 1 (every digit q_j - 1), c1 = 0 (closed form: (sigma(c0), 0)), a key of all q_t - 1; random_kswitch_key;
* memory: sentinel ciphertexts on both sides of d_out, d_in re-read unchanged;
* a key installed again is followed (and permuted again); one digit lift per chunk whatever n_elts, one key product per (chunk,
  non-identity element), he355_path_stats untouched, he355_hoist_release_keys brings the bytes to zero and the next call is still right;
* the plain sum equals the composed sum bit for bit (step 0 included); with real keys a 16-diagonal matrix decodes to numpy's product
  (CKKS: within rotate_hoisted_ref.CKKS_ERROR_CAP x the error of the same sum over he355_rotate; BFV: exactly);
* BFV with real keys: he355_decrypt of the hoisted outputs equals that of he355_rotate; the noise budgets of both are printed, budget > 0.
Layouts and rings beyond this table -- the special prime in the fp64 engine, N = 16384 and 32768 through every call, explicit moduli, L = 1
under K = 5, more Galois elements -- live in tests/test_gpu_hoisted_layouts.py (the table: tests/hoisted_layouts.py)."""
import os
import zlib

import numpy as np
import pytest

import rotate_hoisted_ref as ref
from bfv_gpu_helpers import SENT, At, be, inner_of, refused, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

CKKS = {
    # name: (N, key-level bit sizes, force_u64): the table of tests/test_gpu_parity.py
    "n1024_mixed": (1024, [50, 40, 40, 50], False),
    "n2048_two_primes": (2048, [45, 52], False),
    "n4096_u64_forced": (4096, [60, 45, 45, 60], True),
    "n8192_default": (8192, [60, 45, 60], False),
}
BFV = {"n1024": (1024, [50, 40, 40, 50], 20), "n2048": (2048, [60, 40, 60], 20)}
STEPS = (1, 3, -2)


def make_ckks(be, oracle, N, bits, force=False, primes=None):
    """primes: the moduli themselves, the special prime last (`bits` is not read)"""
    how = {"primes": list(primes)} if primes is not None else {"bit_sizes": bits, "sec128": False}
    if force:
        os.environ["HE355_FORCE_U64"] = "1"
    try:
        g = be.Context(be.SCHEME_CKKS, N, device=0, **how)
    finally:
        os.environ.pop("HE355_FORCE_U64", None)
    o = oracle.Context(oracle.SCHEME_CKKS, N, **how)
    assert g.moduli == o.moduli and (not force or not any(g.fp64))
    return g, o


def make_bfv(be, oracle, N, bits, pb):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    assert g.moduli == o.moduli and g.t == o.t
    return g, o


def random_keys(g, o, rng, steps=STEPS, conj=True):
    """{elt: random key}, set on the device: the elements of `steps` and 2N - 1"""
    keys = {}
    for e in [o.galois_elt(s) for s in steps] + ([2 * o.N - 1] if conj else []):
        keys[e] = o.random_kswitch_key(rng)
        g.set_galois_key(e, keys[e])
    return keys


def rand_cts(o, rng, n, L):
    return np.stack([o.random_poly(rng, L, 2) for _ in range(n)])


def run(g, L, cts, elts, ntt_form, steps=None):
    """the device call between sentinels; d_in is re-read unchanged.  -> [n_elts][n][2][L][N]"""
    n, N = len(cts), g.N
    k = len(steps if steps is not None else elts)
    d_in = g.to_device(cts)
    d_out = sentinelled(g, k * n * 2 * L * N, N)
    at = At(d_out, N)
    if steps is not None:
        g.rotate_hoisted(L, n, d_in, steps, at, ntt_form)
    else:
        g.apply_galois_hoisted(L, n, d_in, elts, at, ntt_form)
    got = inner_of(d_out, N, "d_out").reshape(k, n, 2, L, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    d_in.free()
    d_out.free()
    return got


def check(g, o, L, cts, elts, keys, ntt_form, what):
    got = run(g, L, cts, elts, ntt_form)
    want = ref.hoisted_many(o, cts, elts, keys, ntt_form)
    for r in range(len(elts)):
        for i in range(len(cts)):
            assert np.array_equal(got[r, i], want[r, i]), (what, "element", elts[r], "ciphertext", i)
    return got


def levels(g):
    return [g.L] + ([g.L - 1] if g.L > 1 else [])


@pytest.fixture(scope="module", params=list(CKKS))
def ckks(request, be, oracle):
    N, bits, force = CKKS[request.param]
    g, o = make_ckks(be, oracle, N, bits, force)
    rng = np.random.default_rng(zlib.crc32(request.param.encode()))
    yield g, o, rng, random_keys(g, o, rng)
    g.close()


@pytest.fixture(scope="module", params=list(BFV))
def bfv(request, be, oracle):
    g, o = make_bfv(be, oracle, *BFV[request.param])
    rng = np.random.default_rng(zlib.crc32(request.param.encode()) + 1)
    yield g, o, rng, random_keys(g, o, rng)
    g.close()


def element_set(o):
    e1, e3, em2 = (o.galois_elt(s) for s in STEPS)
    return [e1, e3, em2, 2 * o.N - 1, 1, e3]


def test_ckks_parity(ckks):
    g, o, rng, keys = ckks
    elts = element_set(o)
    for L in levels(g):
        for n in (1, 3):
            check(g, o, L, rand_cts(o, rng, n, L), elts, keys, 1, ("ckks", L, n))
        check(g, o, L, rand_cts(o, rng, 1, L), [elts[2]], keys, 1, ("ckks one element", L))
        # the bits are the library's own, not apply_galois's; by steps: the same call
        cts = rand_cts(o, rng, 1, L)
        got = run(g, L, cts, None, 1, steps=[1, 0, -2])
        assert np.array_equal(got, ref.hoisted_many(o, cts, [elts[0], 1, elts[2]], keys, 1)), ("steps", L)
        assert not np.array_equal(got[0, 0], o.apply_galois(cts[0], elts[0], keys[elts[0]])), L


def test_ckks_parity_n16384(be, oracle):
    g, o = make_ckks(be, oracle, 16384, [60, 45, 45, 45, 60])
    rng = np.random.default_rng(16384)
    keys = random_keys(g, o, rng, steps=(1,))
    check(g, o, g.L, rand_cts(o, rng, 1, g.L), [o.galois_elt(1), 2 * o.N - 1, 1], keys, 1, "n16384")
    g.close()


@pytest.mark.parametrize("ntt_form", [0, 1])
def test_bfv_parity(bfv, ntt_form):
    g, o, rng, keys = bfv
    elts = element_set(o)
    for L in levels(g):
        for n in (1, 3):
            check(g, o, L, rand_cts(o, rng, n, L), elts, keys, ntt_form, ("bfv", ntt_form, L, n))
        check(g, o, L, rand_cts(o, rng, 1, L), [elts[3]], keys, ntt_form, ("bfv one element", ntt_form, L))


def _chunked(g, o, rng, keys, ntt_form):
    """n = 5 under set_chunk(2): three chunks, the slab reused, a ragged last chunk; the counters"""
    elts = element_set(o)
    keyed = sum(e != 1 for e in elts)
    g.set_chunk(2)
    try:
        g.hoist_stats(reset=True)
        paths = g.path_stats()
        check(g, o, g.L, rand_cts(o, rng, 5, g.L), elts, keys, ntt_form, ("chunks", ntt_form))
        st = g.hoist_stats()
        assert st["digit_lifts"] == 3 and st["key_products"] == 3 * keyed, st
        assert g.path_stats() == paths
        g.hoist_stats(reset=True)
        check(g, o, g.L, rand_cts(o, rng, 3, g.L), [1, 1], keys, ntt_form, ("identities", ntt_form))  # nothing to lift
        st = g.hoist_stats()
        assert st["digit_lifts"] == 0 and st["key_products"] == 0, st
    finally:
        g.set_chunk(1024)


def test_ckks_chunks_and_counters(ckks):
    g, o, rng, keys = ckks
    _chunked(g, o, rng, keys, 1)


@pytest.mark.parametrize("ntt_form", [0, 1])
def test_bfv_chunks_and_counters(bfv, ntt_form):
    g, o, rng, keys = bfv
    _chunked(g, o, rng, keys, ntt_form)


def _edges(g, o, rng, keys, ntt_form, sigma_form):
    L, N = g.L, o.N
    elts = element_set(o)[:4]
    full = np.stack([np.stack([np.full(N, q - 1, dtype=np.uint64) for q in o.moduli[:L]])] * 2)
    cts = np.stack([full, rand_cts(o, rng, 1, L)[0]])
    check(g, o, L, cts, elts, keys, ntt_form, "all q - 1")
    # c1 = 0: the key switch of zero is zero, whatever the key: (sigma(c0), 0)
    z = rand_cts(o, rng, 2, L)
    z[:, 1] = 0
    got = run(g, L, z, elts, ntt_form)
    for r, e in enumerate(elts):
        for i in range(2):
            assert not got[r, i, 1].any(), ("c1 = 0", e)
            for j in range(L):
                x = z[i, 0, j]
                if sigma_form != ntt_form:  # NTT-form BFV ciphertexts: sigma acts on the coefficients
                    want = o.ntt(j, o.apply_galois_poly(j, e, 0, o.intt(j, x)))
                else:
                    want = o.apply_galois_poly(j, e, sigma_form, x)
                assert np.array_equal(got[r, i, 0, j], want), ("c1 = 0", e, j)
    # a key of all q_t - 1
    e = elts[0]
    top = np.empty_like(keys[e])
    for t, q in enumerate(o.moduli):
        top[:, :, t, :] = q - 1
    g.set_galois_key(e, top)
    try:
        check(g, o, L, cts, [e, 1], {e: top}, ntt_form, "key of all q - 1")
    finally:
        g.set_galois_key(e, keys[e])


def test_ckks_edge_operands(ckks):
    g, o, rng, keys = ckks
    _edges(g, o, rng, keys, 1, 1)


@pytest.mark.parametrize("ntt_form", [0, 1])
def test_bfv_edge_operands(bfv, ntt_form):
    g, o, rng, keys = bfv
    _edges(g, o, rng, keys, ntt_form, 0)


def test_key_reinstall_release_and_refusals(be, oracle):
    g, o = make_ckks(be, oracle, 2048, [46, 40, 40, 46])
    rng = np.random.default_rng(77)
    L, N = g.L, o.N
    e1, e3 = o.galois_elt(1), o.galois_elt(3)
    cts = rand_cts(o, rng, 2, L)
    d_in, d_out = g.to_device(cts), g.alloc(2 * 2 * 2 * L * N)
    refused(be, lambda: g.apply_galois_hoisted(L, 2, d_in, [e1], d_out))  # "Galois key not present"
    g.apply_galois_hoisted(L, 2, d_in, [1, 1], d_out)                    # the identity needs none
    assert np.array_equal(d_out.download((2, 2, 2, L, N)), np.stack([cts, cts]))
    keys = random_keys(g, o, rng, steps=(1, 3), conj=False)
    refused(be, lambda: g.apply_galois_hoisted(L, 2, d_in, [e1, 2 * N - 1], d_out))  # one of two is missing: nothing runs
    assert g.hoist_stats()["keys_permuted"] == 0
    check(g, o, L, cts, [e1, e3], keys, 1, "first use")
    st = g.hoist_stats()
    assert st["keys_permuted"] == 2 and st["key_bytes"] > 2 * keys[e1].nbytes - 1, st
    check(g, o, L, cts, [e3, e1], keys, 1, "second use")
    assert g.hoist_stats()["keys_permuted"] == 2  # kept per element
    key2 = o.random_kswitch_key(rng)
    g.set_galois_key(e1, key2)
    check(g, o, L, cts, [e1, e3], {e1: key2, e3: keys[e3]}, 1, "after the key was installed again")
    assert g.hoist_stats()["keys_permuted"] == 3
    # the ordinary rotation is untouched by the copies
    g.apply_galois(L, 2, d_in, e1, d_out)
    assert np.array_equal(d_out.download_head((2, 2, L, N)), np.stack([o.apply_galois(c, e1, key2) for c in cts]))
    g.hoist_release_keys()
    st = g.hoist_stats()
    assert st["key_bytes"] == 0 and st["keys_permuted"] == 3, st
    check(g, o, L, cts, [e1, e3], {e1: key2, e3: keys[e3]}, 1, "after the release")
    st = g.hoist_stats()
    assert st["keys_permuted"] == 5 and st["key_bytes"] > 0, st
    # n == 0 and n_elts == 0 touch nothing
    sent = g.to_device(np.full(2 * 2 * L * N, SENT, dtype=np.uint64))
    g.apply_galois_hoisted(L, 0, d_in, [e1], sent)
    g.apply_galois_hoisted(L, 2, d_in, [], sent)
    g.rotate_hoisted_plain_sum(L, 2, d_in, [], d_in, sent)
    assert (sent.download() == SENT).all()
    refused(be, lambda: g.apply_galois_hoisted(L, 2, d_in, [e1], d_in))  # in place
    g.close()


def _plain_sum_parity(g, o, rng, keys, n):
    L, N = g.L, o.N
    steps = [0, 1, -2, 3, 1]
    cts = rand_cts(o, rng, n, L)
    plains = np.stack([o.random_poly(rng, L, 1)[0] for _ in steps])
    d_in, d_pt = g.to_device(cts), g.to_device(plains)
    d_out = sentinelled(g, n * 2 * L * N, N)
    at = At(d_out, N)
    g.rotate_hoisted_plain_sum(L, n, d_in, steps, d_pt, at)
    got = inner_of(d_out, N, "plain sum").reshape(n, 2, L, N)
    assert np.array_equal(got, ref.plain_sum(o, cts, steps, keys, plains))
    assert np.array_equal(d_in.download(cts.shape), cts) and np.array_equal(d_pt.download(plains.shape), plains)
    # a sum that starts with a keyed element, and one of a single term
    for st in ([3, 0], [-2]):
        g.rotate_hoisted_plain_sum(L, n, d_in, st, d_pt, at)
        assert np.array_equal(inner_of(d_out, N, "plain sum").reshape(n, 2, L, N), ref.plain_sum(o, cts, st, keys, plains[:len(st)])), st
    for b in (d_in, d_pt, d_out):
        b.free()


def test_ckks_plain_sum_parity(ckks):
    g, o, rng, keys = ckks
    _plain_sum_parity(g, o, rng, keys, 3)
    g.set_chunk(2)
    try:
        _plain_sum_parity(g, o, rng, keys, 5)
    finally:
        g.set_chunk(1024)


def test_bfv_plain_sum_parity(bfv):
    g, o, rng, keys = bfv
    _plain_sum_parity(g, o, rng, keys, 3)


def _diagonals(rng, n, count, draw):
    """a cyclic-diagonal matrix of `count` diagonals: M[i][(i + s) % n] = diag_s[i], s < count"""
    diags = draw((count, n))
    M = np.zeros((n, n), dtype=diags.dtype)
    for s in range(count):
        M[np.arange(n), (np.arange(n) + s) % n] = diags[s]
    return diags, M


def test_ckks_real_keys_matrix_vector_product(be, oracle):
    N, bits = 1024, [50, 40, 40, 50]
    g, o = make_ckks(be, oracle, N, bits)
    L, n, scale = g.L, N // 2, 2.0 ** 30
    sk = o.keygen_secret(11)
    pk = o.keygen_public(sk, 12)
    steps = list(range(16))
    for s in steps[1:]:
        g.set_galois_key(o.galois_elt(s), o.keygen_galois(sk, o.galois_elt(s), 100 + s))
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    diags, M = _diagonals(rng, n, 16, lambda shape: rng.uniform(-1, 1, shape))
    ct = o.encrypt(pk, oracle.ckks_encode(o, x, scale), 21)
    plains = np.stack([oracle.ckks_encode(o, d, scale) for d in diags])
    d_in, d_pt, d_out = g.to_device(ct[None]), g.to_device(plains), g.alloc(2 * L * N)
    g.rotate_hoisted_plain_sum(L, 1, d_in, steps, d_pt, d_out)
    got = d_out.download((2, L, N))
    # the same sum over he355_rotate: rotate, multiply_plain, add
    rot, term, acc = g.alloc(2 * L * N), g.alloc(2 * L * N), g.alloc(2 * L * N)
    for s in steps:
        src = d_in
        if s:
            g.rotate(L, 1, d_in, s, rot)
            src = rot
        pt_s = At(d_pt, s * L * N)
        g.multiply_plain(L, 2, 1, src, pt_s, be.Context.pairwise(), term if s else acc)
        if s:
            g.add(L, 2, 1, acc, term, be.Context.pairwise(), acc)
    ordinary = acc.download((2, L, N))
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    want = M @ x
    err_h, err_o = np.abs(dec(got) - want).max(), np.abs(dec(ordinary) - want).max()
    print(f"16 diagonals: ordinary {err_o:.3e} hoisted {err_h:.3e}")
    assert err_o < 1e-2, err_o
    assert err_h <= ref.CKKS_ERROR_CAP * err_o, (err_h, err_o)
    g.close()


def test_bfv_real_keys(be, oracle):
    N, bits, pb = BFV["n2048"]
    g, o = make_bfv(be, oracle, N, bits, pb)
    L, half, t = g.L, N // 2, o.t
    codec = oracle.BatchCodec(N, t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    g.set_secret_key(sk)
    steps = list(range(16))
    for s in steps[1:] + [-2]:
        g.set_galois_key(o.galois_elt(s), o.keygen_galois(sk, o.galois_elt(s), 200 + s))
    g.set_galois_key(2 * N - 1, o.keygen_galois(sk, 2 * N - 1, 199))
    rng = np.random.default_rng(6)
    x = rng.integers(0, t, (3, N))
    cts = np.stack([o.encrypt(pk, codec.encode(v), 41 + i) for i, v in enumerate(x)])
    d_in = g.to_device(cts)
    # decryptions of the hoisted outputs are he355_rotate's, exactly; both noise budgets
    hs = [1, 7, -2]
    elts = [o.galois_elt(s) for s in hs] + [2 * N - 1]
    hoisted, ordinary = g.alloc(4 * 3 * 2 * L * N), g.alloc(4 * 3 * 2 * L * N)
    g.apply_galois_hoisted(L, 3, d_in, elts, hoisted, ntt_form=False)
    for r, e in enumerate(elts):
        blk = At(ordinary, r * 3 * 2 * L * N)
        if r < 3:
            g.rotate(L, 3, d_in, hs[r], blk)
        else:
            g.apply_galois(L, 3, d_in, e, blk)
    ph, po = g.alloc(12 * N), g.alloc(12 * N)
    g.decrypt(L, 2, 12, hoisted, ph)
    g.decrypt(L, 2, 12, ordinary, po)
    assert not np.array_equal(hoisted.download(), ordinary.download())
    assert np.array_equal(ph.download(), po.download())
    dec = codec.decode(ph.download((12, N))[1])  # step 1 of ciphertext 1: both rows rotated left by one
    assert np.array_equal(dec[:half], np.roll(x[1, :half], -1)) and np.array_equal(dec[half:], np.roll(x[1, half:], -1))
    bh, bo = g.bfv_noise_budget(L, 2, 12, hoisted), g.bfv_noise_budget(L, 2, 12, ordinary)
    print("noise budget, hoisted:", bh.tolist(), "ordinary:", bo.tolist())
    assert (bh > 0).all() and (bo > 0).all()
    # a 16-diagonal matrix on each row of the batch, NTT-form ciphertexts: exact
    diags = rng.integers(0, t, (16, N))
    pts = g.to_device(np.stack([codec.encode(d) for d in diags]))
    pts_ntt, ntt_in, out = g.alloc(16 * L * N), g.alloc(3 * 2 * L * N), g.alloc(3 * 2 * L * N)
    g.bfv_plain_to_ntt(L, 16, pts, pts_ntt)
    g.bfv_transform_to_ntt(L, 2, 3, d_in, ntt_in)
    g.rotate_hoisted_plain_sum(L, 3, ntt_in, steps, pts_ntt, out)
    g.bfv_transform_from_ntt(L, 2, 3, out, out)
    pm = g.alloc(3 * N)
    g.decrypt(L, 2, 3, out, pm)
    assert (g.bfv_noise_budget(L, 2, 3, out) > 0).all()
    got = pm.download((3, N))
    for i in range(3):
        want = np.zeros(N, dtype=object)
        for s in steps:
            for lo in (0, half):
                want[lo:lo + half] += diags[s, lo:lo + half].astype(object) * np.roll(x[i, lo:lo + half], -s).astype(object)
        assert np.array_equal(codec.decode(got[i]).astype(object) % t, want % t), i
    g.close()
