"""GPU tests of the lazy-mod-down plain sum (run with -m gpu on an MI355X): he355_rotate_hoisted_plain_sum_lazy and
he355_plain_extend_special against their definition in tests/rotate_hoisted_lazy_ref.py -- Python integers and the oracle's transforms --
bit for bit (np.array_equal, no tolerance), and with real keys against the eager sum's plaintexts.

* contexts: the CKKS / BFV tables of tests/test_gpu_rotate_hoisted.py -- N = 1024 (one row per polynomial: the special prime's inverse row pass
  was the whole transform), 2048 {45,52} (L = 1, one digit, the special prime in the other engine), 4096 with the u64 engine forced, 8192
  {60,45,60} (eight rows); BFV N = 1024 and 2048 as random NTT-form residues and, with real keys, through bfv_transform_to_ntt; levels L_top
  and L_top - 1;
* sums [0, 1, -2, 3, 1], [3, 0] (starts keyed: polynomial 1 of B is zeroed by it), [-2], [0], [0, 0], and the all-ones anchor against
  rotate_hoisted_ref.hoisted; n = 1, 3, and 5 under set_chunk(2) (three chunks, a ragged last one, the accumulators reused);
* mod_downs = chunks for the lazy call and = key_products for the eager call; he355_path_stats untouched;
* sentinels on both sides of d_out; d_in and d_plain_qp re-read unchanged;
* ciphertexts and plaintexts all q_i - 1, c1 = 0, a key of all q_t - 1; a key installed again is followed;
* he355_plain_extend_special on CKKS-encoded and BFV plaintexts, the mismatch count on a planted plaintext;
* the two real-key cases of tests/test_rotate_hoisted_lazy_ref_cpu.py through the device, the plaintexts extended on the device.
Layouts and rings beyond that table (an fp64 special prime, N = 16384 and 32768, explicit moduli, L = 1 under K = 5) live in
tests/test_gpu_hoisted_layouts.py (the table: tests/hoisted_layouts.py)."""
import zlib

import numpy as np
import pytest

import rotate_hoisted_lazy_ref as lazy
import rotate_hoisted_ref as ref
from bfv_gpu_helpers import SENT, At, be, inner_of, refused, sentinelled  # noqa: F401 (be: the fixture)
from test_gpu_rotate_hoisted import BFV, CKKS, levels, make_bfv, make_ckks, rand_cts, random_keys

pytestmark = pytest.mark.gpu

STEPS = [0, 1, -2, 3, 1]
CONTEXTS = [("ckks", k) for k in CKKS] + [("bfv", k) for k in BFV]


@pytest.fixture(scope="module", params=CONTEXTS, ids=["-".join(c) for c in CONTEXTS])
def ctx(request, be, oracle):
    scheme, name = request.param
    if scheme == "ckks":
        N, bits, force = CKKS[name]
        g, o = make_ckks(be, oracle, N, bits, force)
    else:
        g, o = make_bfv(be, oracle, *BFV[name])
    rng = np.random.default_rng(zlib.crc32(("lazy" + scheme + name).encode()))
    yield g, o, rng, random_keys(g, o, rng, conj=False)
    g.close()


def rand_qp(o, rng, L, count):
    return np.stack([o.random_poly(rng, L, 1, special=True)[0] for _ in range(count)])


def run(g, L, cts, steps, plain_qp):
    """the device call between sentinels; d_in and d_plain_qp are re-read unchanged.  -> [n][2][L][N]"""
    n, N = len(cts), g.N
    d_in, d_pt = g.to_device(cts), g.to_device(plain_qp)
    d_out = sentinelled(g, n * 2 * L * N, N)
    g.rotate_hoisted_plain_sum_lazy(L, n, d_in, steps, d_pt, At(d_out, N))
    got = inner_of(d_out, N, "d_out").reshape(n, 2, L, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    assert np.array_equal(d_pt.download(plain_qp.shape), plain_qp), "d_plain_qp"
    for b in (d_in, d_pt, d_out):
        b.free()
    return got


def check(g, o, L, cts, steps, keys, plain_qp, what):
    got = run(g, L, cts, steps, plain_qp)
    want = lazy.plain_sum_lazy(o, cts, steps, keys, plain_qp)
    for i in range(len(cts)):
        assert np.array_equal(got[i], want[i]), (what, steps, "ciphertext", i)
    return got


def test_sums(ctx):
    g, o, rng, keys = ctx
    for L in levels(g):
        cts = rand_cts(o, rng, 3, L)
        plain_qp = rand_qp(o, rng, L, len(STEPS))
        check(g, o, L, cts, STEPS, keys, plain_qp, ("n = 3", L))
        for steps in ([3, 0], [-2], [0], [0, 0]):
            check(g, o, L, cts[:1], steps, keys, plain_qp[:len(steps)], ("n = 1", L))
        # the anchor: one keyed step times the all-ones NTT vector is the eager hoisted rotation, bit for bit
        e = o.galois_elt(3)
        got = run(g, L, cts[:1], [3], lazy.ones_qp(o, L)[None])
        assert np.array_equal(got[0], ref.hoisted(o, cts[0], e, keys[e], 1)), ("anchor", L)


def test_chunks_and_stats(ctx):
    g, o, rng, keys = ctx
    L = g.L
    keyed = sum(s != 0 for s in STEPS)
    g.set_chunk(2)
    try:
        g.hoist_stats(reset=True)
        paths = g.path_stats()
        cts = rand_cts(o, rng, 5, L)
        plain_qp = rand_qp(o, rng, L, len(STEPS))
        check(g, o, L, cts, STEPS, keys, plain_qp, "chunks")
        st = g.hoist_stats()
        assert st["digit_lifts"] == 3 and st["key_products"] == 3 * keyed and st["mod_downs"] == 3, st
        g.hoist_stats(reset=True)
        check(g, o, L, cts[:3], [0, 0], keys, plain_qp[:2], "identities")  # nothing to lift, no mod-down
        st = g.hoist_stats()
        assert st["digit_lifts"] == 0 and st["key_products"] == 0 and st["mod_downs"] == 0, st
        # the eager call: one mod-down per key product
        g.hoist_stats(reset=True)
        d_in, d_pt, d_out = g.to_device(cts), g.to_device(np.ascontiguousarray(plain_qp[:, :L])), g.alloc(5 * 2 * L * g.N)
        g.rotate_hoisted_plain_sum(L, 5, d_in, STEPS, d_pt, d_out)
        st = g.hoist_stats()
        assert st["key_products"] == 3 * keyed and st["mod_downs"] == st["key_products"], st
        assert g.path_stats() == paths
        for b in (d_in, d_pt, d_out):
            b.free()
    finally:
        g.set_chunk(1024)


def test_edge_operands(ctx):
    g, o, rng, keys = ctx
    L, N = g.L, o.N
    full = np.stack([np.stack([np.full(N, q - 1, dtype=np.uint64) for q in o.moduli[:L]])] * 2)
    full_qp = np.stack([np.stack([np.full(N, q - 1, dtype=np.uint64) for q in o.moduli[:L] + [o.moduli[-1]]])] * len(STEPS))
    cts = np.stack([full, rand_cts(o, rng, 1, L)[0]])
    check(g, o, L, cts, STEPS, keys, full_qp, "all q - 1")
    # c1 = 0: the key products are zero whatever the keys, the sum is B alone
    z = rand_cts(o, rng, 1, L)
    z[:, 1] = 0
    plain_qp = rand_qp(o, rng, L, 2)
    got = check(g, o, L, z, [3, 1], keys, plain_qp, "c1 = 0")
    assert not got[0, 1].any()
    # a key of all q_t - 1
    e = o.galois_elt(1)
    top = np.empty_like(keys[e])
    for t, q in enumerate(o.moduli):
        top[:, :, t, :] = q - 1
    g.set_galois_key(e, top)
    try:
        check(g, o, L, cts, [1, 0], {e: top}, full_qp[:2], "key of all q - 1")
    finally:
        g.set_galois_key(e, keys[e])


def test_key_reinstall_and_refusals(be, oracle):
    g, o = make_ckks(be, oracle, 2048, [46, 40, 40, 46])
    rng = np.random.default_rng(78)
    L, N = g.L, o.N
    cts = rand_cts(o, rng, 2, L)
    plain_qp = rand_qp(o, rng, L, 2)
    d_in, d_pt, d_out = g.to_device(cts), g.to_device(plain_qp), g.alloc(2 * 2 * L * N)
    refused(be, lambda: g.rotate_hoisted_plain_sum_lazy(L, 2, d_in, [1, 0], d_pt, d_out))  # "Galois key not present"
    assert g.hoist_stats()["keys_permuted"] == 0
    keys = random_keys(g, o, rng, steps=(1, 3), conj=False)
    check(g, o, L, cts, [1, 3], keys, plain_qp, "first use")
    assert g.hoist_stats()["keys_permuted"] == 2
    e1 = o.galois_elt(1)
    key2 = o.random_kswitch_key(rng)
    g.set_galois_key(e1, key2)
    check(g, o, L, cts, [1, 3], {e1: key2, o.galois_elt(3): keys[o.galois_elt(3)]}, plain_qp, "after the key was installed again")
    assert g.hoist_stats()["keys_permuted"] == 3
    # n == 0 and n_steps == 0 touch nothing; in place is refused
    sent = g.to_device(np.full(2 * 2 * L * N, SENT, dtype=np.uint64))
    g.rotate_hoisted_plain_sum_lazy(L, 0, d_in, [1], d_pt, sent)
    g.rotate_hoisted_plain_sum_lazy(L, 2, d_in, [], d_pt, sent)
    g.plain_extend_special(L, 0, d_pt, sent)
    assert (sent.download() == SENT).all()
    refused(be, lambda: g.rotate_hoisted_plain_sum_lazy(L, 2, d_in, [1], d_pt, d_in))
    refused(be, lambda: g.plain_extend_special(L, 2, d_pt, d_pt))
    g.close()


def extend(g, L, plains, check_mismatch):
    """he355_plain_extend_special between sentinels -> ([n][L + 1][N], mismatch or None); the source is re-read unchanged"""
    n, N = len(plains), g.N
    d_src = g.to_device(plains)
    d_dst = sentinelled(g, n * (L + 1) * N, N)
    d_bad = g.to_device(np.full(1, SENT, dtype=np.uint64)) if check_mismatch else None
    g.plain_extend_special(L, n, d_src, At(d_dst, N), d_bad)
    got = inner_of(d_dst, N, "d_plain_qp").reshape(n, L + 1, N)
    assert np.array_equal(d_src.download(plains.shape), plains), "d_plain_ntt"
    bad = int(d_bad.download()[0]) if check_mismatch else None
    for b in (d_src, d_dst) + ((d_bad,) if check_mismatch else ()):
        b.free()
    return got, bad


def test_plain_extend_special(ctx, oracle):
    g, o, rng, _ = ctx
    N, q0 = o.N, o.moduli[0]
    ckks = o.scheme == oracle.SCHEME_CKKS
    for L in levels(g):
        if ckks:
            plains = np.stack([oracle.ckks_encode(o, rng.uniform(-1, 1, N // 2), 2.0 ** 30, L) for _ in range(3)])
        else:
            m = rng.integers(0, o.t, (3, N)).astype(object)
            m = np.where(m > o.t // 2, m - o.t, m)
            plains = np.stack([np.stack([o.ntt(i, (c % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])]) for c in m])
        # a planted coefficient of floor(q_0 / 2) + 5 in the last plaintext: prime 0 reads it as negative
        c = np.zeros(N, dtype=object)
        c[7], c[N - 1] = q0 // 2 + 5, -3
        planted = np.stack([o.ntt(i, (c % q).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])])
        want = [lazy.extend_special(o, p) for p in plains]
        for with_check in (True, False):
            got, bad = extend(g, L, plains, with_check)
            for i in range(3):
                assert np.array_equal(got[i], want[i][0]), (L, i, with_check)
            assert bad == (0 if with_check else None), (L, bad)
        got, bad = extend(g, L, np.concatenate([plains, planted[None]]), True)
        w, wb = lazy.extend_special(o, planted)
        assert np.array_equal(got[3], w) and bad == wb and (bad > 0) == (L >= 2), (L, bad, wb)


def _diagonals(n, count, diags):
    M = np.zeros((n, n), dtype=diags.dtype)
    for s in range(count):
        M[np.arange(n), (np.arange(n) + s) % n] = diags[s]
    return M


def test_ckks_real_keys_sixteen_diagonals(be, oracle):
    N, bits = 1024, [50, 40, 40, 50]
    g, o = make_ckks(be, oracle, N, bits)
    L, n, scale = g.L, N // 2, 2.0 ** 30
    sk = o.keygen_secret(11)
    pk = o.keygen_public(sk, 12)
    steps = list(range(16))
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), 100 + s) for s in steps[1:]}
    for e, k in keys.items():
        g.set_galois_key(e, k)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    diags = rng.uniform(-1, 1, (16, n))
    want = _diagonals(n, 16, diags) @ x
    ct = o.encrypt(pk, oracle.ckks_encode(o, x, scale), 21)
    plains = np.stack([oracle.ckks_encode(o, d, scale) for d in diags])
    d_in, d_pt = g.to_device(ct[None]), g.to_device(plains)
    d_qp, d_bad, d_out, d_eager = g.alloc(16 * (L + 1) * N), g.alloc(1), g.alloc(2 * L * N), g.alloc(2 * L * N)
    g.plain_extend_special(L, 16, d_pt, d_qp, d_bad)
    assert int(d_bad.download()[0]) == 0
    g.rotate_hoisted_plain_sum_lazy(L, 1, d_in, steps, d_qp, d_out)
    g.rotate_hoisted_plain_sum(L, 1, d_in, steps, d_pt, d_eager)
    got, eager = d_out.download((2, L, N)), d_eager.download((2, L, N))
    assert np.array_equal(got, lazy.plain_sum_lazy(o, ct[None], steps, keys, d_qp.download((16, L + 1, N)))[0])
    assert not np.array_equal(got, eager)
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    err_l, err_e = np.abs(dec(got) - want).max(), np.abs(dec(eager) - want).max()
    print(f"16 diagonals: eager {err_e:.3e} lazy {err_l:.3e}")
    assert err_e < 1e-2, err_e
    assert err_l <= ref.CKKS_ERROR_CAP * err_e, (err_l, err_e)
    g.close()


def test_bfv_real_keys_five_terms(be, oracle):
    N, bits, pb = BFV["n2048"]
    g, o = make_bfv(be, oracle, N, bits, pb)
    L, half, t = g.L, N // 2, o.t
    codec = oracle.BatchCodec(N, t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    g.set_secret_key(sk)
    for s in set(STEPS) - {0}:
        g.set_galois_key(o.galois_elt(s), o.keygen_galois(sk, o.galois_elt(s), 200 + s))
    rng = np.random.default_rng(6)
    x = rng.integers(0, t, (3, N))
    diags = rng.integers(0, t, (len(STEPS), N))
    cts = np.stack([o.encrypt(pk, codec.encode(v), 41 + i) for i, v in enumerate(x)])
    d_in, pts = g.to_device(cts), g.to_device(np.stack([codec.encode(d) for d in diags]))
    R = len(STEPS)
    pts_ntt, pts_qp, d_bad = g.alloc(R * L * N), g.alloc(R * (L + 1) * N), g.alloc(1)
    ntt_in, out, eager = g.alloc(3 * 2 * L * N), g.alloc(3 * 2 * L * N), g.alloc(3 * 2 * L * N)
    g.bfv_plain_to_ntt(L, R, pts, pts_ntt)
    g.plain_extend_special(L, R, pts_ntt, pts_qp, d_bad)
    assert int(d_bad.download()[0]) == 0
    g.bfv_transform_to_ntt(L, 2, 3, d_in, ntt_in)
    g.rotate_hoisted_plain_sum_lazy(L, 3, ntt_in, STEPS, pts_qp, out)
    g.rotate_hoisted_plain_sum(L, 3, ntt_in, STEPS, pts_ntt, eager)
    assert not np.array_equal(out.download(), eager.download())
    g.bfv_transform_from_ntt(L, 2, 3, out, out)
    g.bfv_transform_from_ntt(L, 2, 3, eager, eager)
    pm, pe = g.alloc(3 * N), g.alloc(3 * N)
    g.decrypt(L, 2, 3, out, pm)
    g.decrypt(L, 2, 3, eager, pe)
    b_l, b_e = g.bfv_noise_budget(L, 2, 3, out), g.bfv_noise_budget(L, 2, 3, eager)
    print("noise budget, lazy:", b_l.tolist(), "eager:", b_e.tolist())
    assert (b_l > 0).all() and (b_e > 0).all()
    got = pm.download((3, N))
    assert np.array_equal(got, pe.download((3, N)))
    for i in range(3):
        want = np.zeros(N, dtype=object)
        for s, d in zip(STEPS, diags):
            for lo in (0, half):
                want[lo:lo + half] += d[lo:lo + half].astype(object) * np.roll(x[i, lo:lo + half], -s).astype(object)
        assert np.array_equal(codec.decode(got[i]).astype(object) % t, want % t), i
    g.close()
