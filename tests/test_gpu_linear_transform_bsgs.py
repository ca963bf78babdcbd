"""GPU tests of the baby-step/giant-step linear transform (run with -m gpu on an MI355X): he355_linear_transform_bsgs against its definition
in tests/linear_transform_bsgs_ref.py -- Python integers and the oracle's transforms -- bit for bit (np.array_equal, no tolerance).

* contexts: the CKKS / BFV tables of tests/test_gpu_rotate_hoisted.py with the default random keys (steps 1, 3, -2) -- N = 1024 {50,40,40,50}
  (one row per polynomial: the special prime's row pass is the whole transform), 2048 {45,52} (L = 1, one digit, P in the other engine), 4096
  with the u64 engine forced, 8192 {60,45,60}; BFV N = 1024 and 2048 as NTT-form residues; levels L_top and L_top - 1;
* splits: baby [0, 1, -2] x giant [0, 3]; giant [3, 0] (the accumulator starts keyed); baby [1, -2] x giant [3] (no identity anywhere);
  [0] x [0]; [0, 1] x [0, 3] under masks that drop one term, a whole giant row and a whole baby column -- the column's key is not installed on
  that context, and the full mask is refused there; n = 1, 3, and 5 under set_chunk(2) (three chunks, a ragged last one, the store and blocks reused);
* anchors against existing DEVICE calls, bit for bit: a one-row identity giant is he355_rotate_hoisted_plain_sum_lazy over the baby steps; a
  one-column identity baby with all-ones plaintexts is that call over the giant steps;
* the run boundary on the device: N = 1024 {60,40,60} -- the 60-bit primes are the ones whose 128-bit sums fill up, after 256 terms -- with
  258 identity babies and one keyed one, operands all q_i - 1, one ciphertext;
* four calls back to back with different splits and masks and no sync between them: each is the reference (the term tables do not race);
* a used step without its key: "he355_linear_transform_bsgs: Galois key not present";
* ciphertexts and plaintexts all q_i - 1, c1 = 0, a key of all q_t - 1; a key installed again is followed;
* counters: digit_lifts, key_products, mod_downs (one per used keyed giant row and one last one, per chunk) and inner_sums by their rules,
  he355_path_stats unchanged;
* sentinels on both sides of d_out; d_in and d_plain_qp re-read unchanged; he355_linear_transform_bsgs_scratch_bytes is at least the pool
  growth he355_alloc_stats sees across the call;
* the two real-key cases of tests/test_linear_transform_bsgs_ref_cpu.py through the device, the plaintexts extended by
  he355_plain_extend_special.
Layouts and rings beyond that table (an fp64 special prime, N = 16384 and 32768, explicit moduli, L = 1 under K = 5), a second fold of the
inner sum and folds under 14- to 31-bit moduli live in tests/test_gpu_hoisted_layouts.py (the table: tests/hoisted_layouts.py)."""
import zlib

import numpy as np
import pytest

import linear_transform_bsgs_ref as bsgs
import rotate_hoisted_lazy_ref as lazy
from bfv_gpu_helpers import SENT, At, be, inner_of, refused, sentinelled  # noqa: F401 (be: the fixture)
from test_gpu_rotate_hoisted import BFV, CKKS, levels, make_bfv, make_ckks, rand_cts, random_keys
from test_linear_transform_bsgs_ref_cpu import BABY, CKKS_RATIO_CAP, GIANT
from test_rotate_hoisted_lazy_ref_cpu import _diagonals

pytestmark = pytest.mark.gpu

CONTEXTS = [("ckks", k) for k in CKKS] + [("bfv", k) for k in BFV]


@pytest.fixture(scope="module", params=CONTEXTS, ids=["-".join(c) for c in CONTEXTS])
def ctx(request, be, oracle):
    scheme, name = request.param
    if scheme == "ckks":
        N, bits, force = CKKS[name]
        g, o = make_ckks(be, oracle, N, bits, force)
    else:
        g, o = make_bfv(be, oracle, *BFV[name])
    rng = np.random.default_rng(zlib.crc32(("bsgs" + scheme + name).encode()))
    yield g, o, rng, random_keys(g, o, rng, conj=False)
    g.close()


def rand_qp(o, rng, L, n_giant, n_baby):
    return np.stack([o.random_poly(rng, L, 1, special=True)[0] for _ in range(n_giant * n_baby)]).reshape(n_giant, n_baby, L + 1, o.N)


def full_cts(o, L, n=1):
    return np.stack([np.stack([np.stack([np.full(o.N, q - 1, dtype=np.uint64) for q in o.moduli[:L]])] * 2)] * n)


def full_qp(o, L, n_giant, n_baby):
    one = np.stack([np.full(o.N, q - 1, dtype=np.uint64) for q in o.moduli[:L] + [o.moduli[-1]]])
    return np.broadcast_to(one, (n_giant, n_baby, L + 1, o.N)).copy()


def run(g, L, cts, baby, giant, plain_qp, mask=None):
    """the device call between sentinels; d_in and d_plain_qp are re-read unchanged.  -> [n][2][L][N]"""
    n, N = len(cts), g.N
    d_in, d_pt = g.to_device(cts), g.to_device(plain_qp)
    d_out = sentinelled(g, n * 2 * L * N, N)
    g.linear_transform_bsgs(L, n, d_in, baby, giant, d_pt, At(d_out, N), mask)
    got = inner_of(d_out, N, "d_out").reshape(n, 2, L, N)
    assert np.array_equal(d_in.download(cts.shape), cts), "d_in"
    assert np.array_equal(d_pt.download(plain_qp.shape), plain_qp), "d_plain_qp"
    for b in (d_in, d_pt, d_out):
        b.free()
    return got


def check(g, o, L, cts, baby, giant, keys, plain_qp, what, mask=None):
    got = run(g, L, cts, baby, giant, plain_qp, mask)
    want = bsgs.linear_transform_bsgs(o, cts, baby, giant, keys, plain_qp, mask)
    for i in range(len(cts)):
        assert np.array_equal(got[i], want[i]), (what, baby, giant, mask, "ciphertext", i)
    return got


def lazy_device(g, L, cts, steps, plain_qp):
    d_in, d_pt, d_out = g.to_device(cts), g.to_device(plain_qp), g.alloc(cts.size)
    g.rotate_hoisted_plain_sum_lazy(L, len(cts), d_in, steps, d_pt, d_out)
    got = d_out.download(cts.shape)
    for b in (d_in, d_pt, d_out):
        b.free()
    return got


def test_splits(ctx):
    g, o, rng, keys = ctx
    for L in levels(g):
        cts = rand_cts(o, rng, 3, L)
        plain_qp = rand_qp(o, rng, L, 2, 3)
        check(g, o, L, cts, [0, 1, -2], [0, 3], keys, plain_qp, ("n = 3", L))
        check(g, o, L, cts[:1], [0, 1, -2], [3, 0], keys, plain_qp, ("starts keyed", L))
        check(g, o, L, cts[:1], [1, -2], [3], keys, plain_qp[:1, :2], ("no identity", L))
        check(g, o, L, cts[:1], [0], [0], keys, plain_qp[:1, :1], ("identities", L))
        for mask in ([[1, 0], [1, 1]], [[1, 1], [0, 0]], [[0, 0], [1, 1]], [[1, 0], [1, 0]], [[0, 1], [0, 1]]):
            check(g, o, L, cts[:1], [0, 1], [0, 3], keys, plain_qp[:, :2], ("mask", L), mask)


def test_anchors_against_the_lazy_device_call(ctx):
    g, o, rng, keys = ctx
    for L in levels(g):
        cts = rand_cts(o, rng, 2, L)
        baby = [0, 1, -2, 3, 1]
        plain_qp = rand_qp(o, rng, L, 1, len(baby))
        assert np.array_equal(run(g, L, cts, baby, [0], plain_qp), lazy_device(g, L, cts, baby, plain_qp[0])), ("one identity giant row", L)
        giant = [3, 0, -2]
        ones = np.stack([lazy.ones_qp(o, L)] * len(giant))
        assert np.array_equal(run(g, L, cts, [0], giant, ones[:, None]), lazy_device(g, L, cts, giant, ones)), ("one identity baby, ones", L)


def test_chunks_and_stats(ctx):
    g, o, rng, keys = ctx
    L = g.L
    baby, giant = [0, 1, -2], [3, 0]  # every used giant row has a keyed baby
    g.set_chunk(2)
    try:
        for n in (1, 3, 5):
            chunks = (n + 1) // 2
            g.hoist_stats(reset=True)
            paths = g.path_stats()
            cts = rand_cts(o, rng, n, L)
            plain_qp = rand_qp(o, rng, L, 2, 3)
            check(g, o, L, cts, baby, giant, keys, plain_qp, ("chunks", n))
            st = g.hoist_stats()
            # per chunk: one lift for the babies and one per keyed giant row; two keyed babies and one keyed row; that row's mod-down and the last one
            assert st["digit_lifts"] == 2 * chunks and st["key_products"] == 3 * chunks and st["mod_downs"] == 2 * chunks and st["inner_sums"] == 2 * chunks, (n, st)
            assert g.path_stats() == paths
        # a masked row and column count nothing: baby 1 and giant 3 are not used
        g.hoist_stats(reset=True)
        check(g, o, L, cts[:3], baby, giant, keys, plain_qp, "masked", [[0, 0, 0], [1, 0, 1]])
        st = g.hoist_stats()
        assert st["digit_lifts"] == 2 and st["key_products"] == 2 and st["mod_downs"] == 2 and st["inner_sums"] == 2, st
    finally:
        g.set_chunk(1024)


def test_edge_operands(ctx):
    g, o, rng, keys = ctx
    L = g.L
    baby, giant = [0, 1, -2], [0, 3]
    cts = np.concatenate([full_cts(o, L), rand_cts(o, rng, 1, L)])
    check(g, o, L, cts, baby, giant, keys, full_qp(o, L, 2, 3), "all q - 1")
    # c1 = 0: the baby key products are zero whatever the keys
    z = rand_cts(o, rng, 1, L)
    z[:, 1] = 0
    check(g, o, L, z, [3, 1], [0, -2], keys, rand_qp(o, rng, L, 2, 2), "c1 = 0")
    # a key of all q_t - 1, as a baby and as a giant step
    e = o.galois_elt(1)
    top = np.empty_like(keys[e])
    for t, q in enumerate(o.moduli):
        top[:, :, t, :] = q - 1
    g.set_galois_key(e, top)
    try:
        check(g, o, L, cts, [1, 0], [0, 1], {e: top}, full_qp(o, L, 2, 2), "key of all q - 1")
    finally:
        g.set_galois_key(e, keys[e])


def test_the_run_boundary_on_the_device(be, oracle):
    g, o = make_ckks(be, oracle, 1024, [60, 40, 60])
    rng = np.random.default_rng(91)
    keys = random_keys(g, o, rng, steps=(1,), conj=False)
    L = g.L
    baby = [0] * 258 + [1]  # 259 terms of (q - 1)^2 under the 60-bit primes: one fold after 256, then three more
    check(g, o, L, full_cts(o, L), baby, [0], keys, full_qp(o, L, 1, len(baby)), "run boundary")
    g.close()


def no_key(be, f):
    """refused with the named message, under the call's name"""
    with pytest.raises(be.HE355Error) as ei:
        f()
    assert ei.value.code == be.E_INVALID_ARGS, ei.value
    assert "he355_linear_transform_bsgs: Galois key not present" in str(ei.value), ei.value


def test_calls_back_to_back_without_a_sync(ctx):
    """two calls with different splits and masks -- different term tables -- queued one behind the other, nothing downloaded in between: each
    is still the reference (the first call's launches read ITS table while the second call's is uploaded)"""
    g, o, rng, keys = ctx
    L, N = g.L, o.N
    cts = rand_cts(o, rng, 3, L)
    plain_qp = rand_qp(o, rng, L, 2, 3)
    jobs = [([0, 1, -2], [3, 0], [[1, 1, 1], [1, 0, 1]], plain_qp), ([1, -2], [0, 3], [[0, 1], [1, 1]], plain_qp[:, :2].copy()),
            ([0, 1, -2], [3, 0], [[0, 0, 1], [1, 1, 0]], plain_qp), ([-2, 0, 1], [3], None, plain_qp[:1])]
    d_in = g.to_device(cts)
    bufs = [(g.to_device(np.ascontiguousarray(pq)), g.alloc(cts.size)) for _, _, _, pq in jobs]
    g.sync()
    for (baby, giant, mask, _), (d_pt, d_out) in zip(jobs, bufs):
        g.linear_transform_bsgs(L, 3, d_in, baby, giant, d_pt, d_out, mask)
    for k, ((baby, giant, mask, pq), (_, d_out)) in enumerate(zip(jobs, bufs)):
        want = bsgs.linear_transform_bsgs(o, cts, baby, giant, keys, np.ascontiguousarray(pq), mask)
        assert np.array_equal(d_out.download(cts.shape), want), ("call", k)
    for b in [d_in] + [x for pair in bufs for x in pair]:
        b.free()


def test_masks_keys_reinstall_and_refusals(be, oracle):
    g, o = make_ckks(be, oracle, 2048, [46, 40, 40, 46])
    rng = np.random.default_rng(79)
    L, N = g.L, o.N
    cts = rand_cts(o, rng, 2, L)
    plain_qp = rand_qp(o, rng, L, 2, 2)
    d_in, d_pt, d_out = g.to_device(cts), g.to_device(plain_qp), g.alloc(2 * 2 * L * N)
    no_key(be, lambda: g.linear_transform_bsgs(L, 2, d_in, [0, 1], [0, 3], d_pt, d_out))
    assert g.hoist_stats()["keys_permuted"] == 0
    # the key of step 3 alone: the baby column of step 1 is masked and needs none; the whole row of step 3 masked needs none at all
    keys = random_keys(g, o, rng, steps=(3,), conj=False)
    check(g, o, L, cts, [0, 1], [0, 3], keys, plain_qp, "column dropped", [[1, 0], [1, 0]])
    no_key(be, lambda: g.linear_transform_bsgs(L, 2, d_in, [0, 1], [0, 3], d_pt, d_out))
    no_key(be, lambda: g.linear_transform_bsgs(L, 2, d_in, [0, 1], [0, 3], d_pt, d_out, [[1, 0], [1, 1]]))
    check(g, o, L, cts, [0, 1], [0, -2], {}, plain_qp, "row and column dropped", [[1, 0], [0, 0]])
    assert g.hoist_stats()["keys_permuted"] == 1
    keys.update(random_keys(g, o, rng, steps=(1,), conj=False))
    check(g, o, L, cts, [0, 1], [0, 3], keys, plain_qp, "first use")
    e1 = o.galois_elt(1)
    keys[e1] = o.random_kswitch_key(rng)
    g.set_galois_key(e1, keys[e1])
    check(g, o, L, cts, [0, 1], [1, 3], keys, plain_qp, "after the key was installed again")
    assert g.hoist_stats()["keys_permuted"] == 3
    # nothing to do touches nothing; in place is refused
    sent = g.to_device(np.full(2 * 2 * L * N, SENT, dtype=np.uint64))
    g.linear_transform_bsgs(L, 0, d_in, [1], [0], d_pt, sent)
    g.linear_transform_bsgs(L, 2, d_in, [], [0], d_pt, sent)
    g.linear_transform_bsgs(L, 2, d_in, [1], [], d_pt, sent)
    assert (sent.download() == SENT).all()
    refused(be, lambda: g.linear_transform_bsgs(L, 2, d_in, [1], [0], d_pt, d_in))
    g.close()


def test_scratch_bytes_bound_the_pool_growth(be, oracle):
    g, o = make_ckks(be, oracle, 2048, [46, 40, 40, 46])
    rng = np.random.default_rng(80)
    keys = random_keys(g, o, rng, conj=False)
    L, N, n = g.L, o.N, 3
    baby, giant = [0, 1, -2], [0, 3]
    cts, plain_qp = rand_cts(o, rng, n, L), rand_qp(o, rng, L, 2, 3)
    d_in, d_pt, d_out = g.to_device(cts), g.to_device(plain_qp), g.alloc(n * 2 * L * N)
    g.rotate_hoisted_plain_sum_lazy(L, n, d_in, baby, g.to_device(plain_qp[0]), d_out)  # the key-switch scratch and the permuted keys exist
    held = lambda s: s["live_bytes"] + s["cached_bytes"]
    before = held(g.alloc_stats())
    g.linear_transform_bsgs(L, n, d_in, baby, giant, d_pt, d_out)
    growth = held(g.alloc_stats()) - before
    bound = g.linear_transform_bsgs_scratch_bytes(L, n, len(baby))
    print(f"pool growth {growth} bytes, scratch bound {bound} bytes")
    assert 0 < growth <= bound, (growth, bound)
    assert np.array_equal(d_out.download(cts.shape), bsgs.linear_transform_bsgs(o, cts, baby, giant, keys, plain_qp))
    g.close()


def test_ckks_real_keys_sixteen_diagonals_four_by_four(be, oracle):
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
    split = bsgs.split_diagonals(diags, BABY, GIANT, lambda v, s: np.roll(v, -s))
    enc = lambda vs: np.stack([oracle.ckks_encode(o, v, scale) for v in vs])
    d_in, d_flat, d_split = g.to_device(ct[None]), g.to_device(enc(diags)), g.to_device(enc([v for row in split for v in row]))
    d_fqp, d_sqp, d_bad = g.alloc(16 * (L + 1) * N), g.alloc(16 * (L + 1) * N), g.alloc(1)
    d_out, d_lazy = g.alloc(2 * L * N), g.alloc(2 * L * N)
    for src, dst in ((d_flat, d_fqp), (d_split, d_sqp)):
        g.plain_extend_special(L, 16, src, dst, d_bad)
        assert int(d_bad.download()[0]) == 0
    g.linear_transform_bsgs(L, 1, d_in, BABY, GIANT, d_sqp, d_out)
    g.rotate_hoisted_plain_sum_lazy(L, 1, d_in, steps, d_fqp, d_lazy)
    got, flat = d_out.download((2, L, N)), d_lazy.download((2, L, N))
    assert np.array_equal(got, bsgs.linear_transform_bsgs(o, ct[None], BABY, GIANT, keys, d_sqp.download((4, 4, L + 1, N)))[0])
    dec = lambda c: oracle.ckks_decode(o, o.decrypt_phase(c, sk), scale * scale)
    err_b, err_f = np.abs(dec(got) - want).max(), np.abs(dec(flat) - want).max()
    print(f"16 diagonals: flat lazy {err_f:.3e} bsgs 4x4 {err_b:.3e} ratio {err_b / err_f:.3f}")
    assert err_f < 1e-2, err_f
    assert err_b <= CKKS_RATIO_CAP * err_f, (err_b, err_f)
    g.close()


def test_bfv_real_keys_sixteen_diagonals_four_by_four(be, oracle):
    N, bits, pb = BFV["n2048"]
    g, o = make_bfv(be, oracle, N, bits, pb)
    L, half, t = g.L, N // 2, o.t
    codec = oracle.BatchCodec(N, t)
    sk = o.keygen_secret(31)
    pk = o.keygen_public(sk, 32)
    g.set_secret_key(sk)
    keys = {o.galois_elt(s): o.keygen_galois(sk, o.galois_elt(s), 200 + s) for s in set(BABY + GIANT) if s}
    for e, k in keys.items():
        g.set_galois_key(e, k)
    rng = np.random.default_rng(6)
    x = rng.integers(0, t, (2, N))
    diags = rng.integers(0, t, (16, N))
    rot = lambda v, s: np.concatenate([np.roll(v[:half], -s), np.roll(v[half:], -s)])
    split = bsgs.split_diagonals(diags, BABY, GIANT, rot)
    cts = np.stack([o.encrypt(pk, codec.encode(v), 41 + i) for i, v in enumerate(x)])
    d_in, pts = g.to_device(cts), g.to_device(np.stack([codec.encode(v) for row in split for v in row]))
    pts_ntt, pts_qp, d_bad = g.alloc(16 * L * N), g.alloc(16 * (L + 1) * N), g.alloc(1)
    ntt_in, out = g.alloc(2 * 2 * L * N), g.alloc(2 * 2 * L * N)
    g.bfv_plain_to_ntt(L, 16, pts, pts_ntt)
    g.plain_extend_special(L, 16, pts_ntt, pts_qp, d_bad)
    assert int(d_bad.download()[0]) == 0
    g.bfv_transform_to_ntt(L, 2, 2, d_in, ntt_in)
    g.linear_transform_bsgs(L, 2, ntt_in, BABY, GIANT, pts_qp, out)
    want_bits = bsgs.linear_transform_bsgs(o, ntt_in.download((2, 2, L, N)), BABY, GIANT, keys, pts_qp.download((4, 4, L + 1, N)))
    assert np.array_equal(out.download((2, 2, L, N)), want_bits)
    g.bfv_transform_from_ntt(L, 2, 2, out, out)
    pm = g.alloc(2 * N)
    g.decrypt(L, 2, 2, out, pm)
    budget = g.bfv_noise_budget(L, 2, 2, out)
    print("noise budget:", budget.tolist())
    assert (budget > 0).all()
    got = pm.download((2, N))
    for i in range(2):
        want = np.zeros(N, dtype=object)
        for s in range(16):
            want += diags[s].astype(object) * rot(x[i], s).astype(object)
        assert np.array_equal(codec.decode(got[i]).astype(object) % t, want % t), i
    g.close()
