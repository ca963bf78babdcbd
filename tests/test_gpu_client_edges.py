"""The client kernels (csrc/he355_kernels_client.hip: CKKS / BFV encoders, encryption, decryption) at structured and extreme operands.

tests/test_gpu_client.py runs them on uniform data in one regime: CKKS coefficients below 2^31, three ciphertexts per call, phases and
dropped residues nowhere near a rounding edge.  Here every operand comes from tests/client_operands.py and every expectation is one of
  * the product's host client (tests/csim: the same inline code, so equality is bit for bit),
  * the mpmath fixture tests/golden/client_edge_vectors.json (CKKS codec: the bounds of tests/test_client_edges_cpu.py),
  * the oracle, and a closed form in Python integers (BFV rounding, encryption under a constant public key).
One context per case, closed in `finally`."""
import importlib

import numpy as np
import pytest

import client_operands as co
import edge_operands as eo
import sampler_np as sn
import shoup_rings as shoup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on the MI355X box")
    return mod


@pytest.fixture(scope="module")
def sim():
    return co.host_sim()


@pytest.fixture(scope="module")
def fixture():
    return co.load_fixture()


def _pair(be, oracle, scheme, N, bits, pb=0):
    ckks = scheme == "ckks"
    g = be.Context(be.SCHEME_CKKS if ckks else be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_CKKS if ckks else oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    assert g.moduli == o.moduli and g.t == o.t
    return g, o


def _f64(buf, shape):
    return buf.download().view(np.float64).reshape(shape)


def _i64(buf, shape):
    return buf.download().view(np.int64).reshape(shape)


# ---- CKKS encode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", co.CKKS_ENCODE_N)
def test_ckks_encode_at_every_input_and_scale(be, sim, oracle, fixture, N):
    """N = 1024: fewer butterflies than the block has threads; N = 4096: the block's strided loops run more than once.  Device == host bit
    for bit, and the device meets the host's two bounds against the exact coefficients."""
    g, o = _pair(be, oracle, "ckks", N, co.CKKS_ENCODE_CHAIN)
    h = co.HostClient(sim, "ckks", N, co.CKKS_ENCODE_CHAIN)
    try:
        L = g.L
        cases = {c["id"]: dict(c, positions=fixture["positions"][str(N)]) for c in fixture["encode"] if c["N"] == N}
        full = [nm for nm in co.CKKS_INPUTS if len(co.ckks_input(nm, N)) == N // 2]
        groups = [full] + [[nm] for nm in co.CKKS_INPUTS if nm not in full]
        assert len(cases) == 3 * len(co.CKKS_INPUTS) and len(groups) == 3
        for names in groups:  # one call per count: the full-width inputs as one batch
            x = np.stack([co.ckks_input(nm, N) for nm in names])
            dv = g.to_device(x.view(np.uint64))
            for scale in co.CKKS_SCALES:
                plain = g.alloc(len(names) * L * N)
                g.ckks_encode(len(names), dv, x.shape[1], scale, plain)
                got = plain.download((len(names), L, N))
                for r, nm in enumerate(names):
                    case = cases[f"{nm}/N{N}/s{int(np.log2(scale))}"]
                    assert co.digest(x[r]) == case["digest"]
                    assert np.array_equal(got[r], h.ckks_encode(x[r], scale)), case["id"]
                    co.check_encode_case(case, co.coeffs_from_plain(o, got[r]), "device")
    finally:
        h.close()
        g.close()


@pytest.mark.parametrize("N", co.CKKS_ENCODE_N)
def test_ckks_encode_refuses_what_does_not_fit_and_recovers(be, sim, oracle, N):
    """a coefficient of 2^63, +inf and NaN raise through the device flag; the flag is cleared per call, so the next valid call on the same
    context succeeds and equals the host"""
    g, o = _pair(be, oracle, "ckks", N, co.CKKS_ENCODE_CHAIN)
    h = co.HostClient(sim, "ckks", N, co.CKKS_ENCODE_CHAIN)
    try:
        L, scale = g.L, 2.0 ** 40
        good = co.ckks_input("uniform", N)
        for name, bad in co.ckks_refused_inputs(N, scale):
            for rows in (np.stack([bad]), np.stack([good, bad, good])):  # alone, and between two valid rows of a batch
                plain = g.alloc(len(rows) * L * N)
                with pytest.raises(be.HE355Error):
                    g.ckks_encode(len(rows), g.to_device(rows.view(np.uint64)), N // 2, scale, plain)
                g.ckks_encode(1, g.to_device(good[None].view(np.uint64)), N // 2, scale, plain)
                assert np.array_equal(plain.download_head((L, N)), h.ckks_encode(good, scale)), name
        # the largest value that is accepted: the constant coefficient 2^62
        ok = np.full(N // 2, 2.0 ** 62 / scale)
        plain = g.alloc(L * N)
        g.ckks_encode(1, g.to_device(ok[None].view(np.uint64)), N // 2, scale, plain)
        got = plain.download((L, N))
        assert np.array_equal(got, h.ckks_encode(ok, scale))
        c0 = [int(o.intt(i, got[i])[0]) for i in range(L)]
        assert c0 == [2 ** 62 % int(o.moduli[i]) for i in range(L)]
    finally:
        h.close()
        g.close()


def test_ckks_encode_negative_multiple_of_a_prime(be, sim, oracle):
    """a coefficient -k q_i reduces to 0 under q_i (the `m == 0` branch, not q_i - 0) and to q_j - (k q_i mod q_j) under the others"""
    N, bits = 1024, co.CKKS_ENCODE_CHAIN
    g, o = _pair(be, oracle, "ckks", N, bits)
    h = co.HostClient(sim, "ckks", N, bits)
    try:
        L = g.L
        rows, picks = co.negative_prime_multiples(o)
        plain = g.alloc(len(rows) * L * N)
        g.ckks_encode(len(rows), g.to_device(rows.view(np.uint64)), N // 2, 1.0, plain)
        got = plain.download((len(rows), L, N))
        for r, (i, k) in enumerate(picks):
            assert np.array_equal(got[r], h.ckks_encode(rows[r], 1.0))
            co.check_negative_prime_multiple(o, got[r], i, k)
    finally:
        h.close()
        g.close()


# ---- CKKS decode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", list(co.DECODE_CHAINS))
def test_ckks_decode_at_every_word_count(be, sim, oracle, fixture, chain):
    """every coefficient family at every level of the chain ({60, 45 x 15, 60}: L = 1 .. 16, so every instantiation W = 3 .. 18 of
    k_ckks_decode_compose launches): device == host bit for bit, within 4 E_np of the exact slots, and decode_slots returns the same bits"""
    N, bits, levels = co.DECODE_CHAINS[chain]
    g, o = _pair(be, oracle, "ckks", N, bits)
    h = co.HostClient(sim, "ckks", N, bits)
    half = N // 2
    ranges = [(0, 3), (half - 2, 2), (half // 2, 1)]
    try:
        by_level = {}
        for L, fam, plain, cases in co.decode_operands(o, chain, fixture):
            by_level.setdefault(L, []).append((fam, plain, cases))
        assert sorted(by_level) == levels
        for L, rows in by_level.items():
            Q = co.prod(o.moduli[:L])
            batch = np.stack([p for _, p, _ in rows])
            dpl = g.to_device(batch)
            seen = set()
            for sname in ("Q", "2^30", "2^90"):  # the whole batch at every scale: what is not a fixture case is still held to the host
                scale = co.decode_scale(sname, Q)
                out = g.alloc(len(rows) * half)
                g.ckks_decode(L, len(rows), dpl, scale, out)
                vals = _f64(out, (len(rows), half))
                for r, (fam, plain, cases) in enumerate(rows):
                    assert np.array_equal(vals[r], h.ckks_decode(plain, scale)), (L, fam, sname)
                    for case in cases:
                        if float.fromhex(case["scale"]) == scale and case["id"].endswith("/" + sname):
                            co.check_decode_case(case, vals[r], "device")
                            seen.add(case["id"])
                tot = sum(c for _, c in ranges)
                outs = g.alloc(len(rows) * tot)
                g.ckks_decode_slots(L, len(rows), dpl, scale, ranges, outs)
                assert np.array_equal(_f64(outs, (len(rows), tot)), np.concatenate([vals[:, f:f + c] for f, c in ranges], axis=1)), (L, sname)
            assert seen == {c["id"] for _, _, cases in rows for c in cases}, L
    finally:
        h.close()
        g.close()


# ---- BFV decrypt ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,levels", [("b60_40_40", [1, 2, 3]), ("b45x15", [1, 15, 16]), ("b50_40_t16", [2]), ("b60x4_t31", [4])])
def test_bfv_decrypt_at_the_planted_phases(be, oracle, chain, levels):
    """round(t x / Q) at the tie points, at x = 0 and x = Q - 1 (result t, which wraps to 0): sizes 2 and 3 under the constant keys 1 and -1
    (phase c0 +- c1 + c2 in closed form) and under a real key; planted and uniform ciphertexts alternate.  L = 16 is the limit of the
    kernel's modulus table."""
    N, bits, pb = co.BFV_DECRYPT_CHAINS[chain]
    g, o = _pair(be, oracle, "bfv", N, bits, pb)
    t = int(o.t)
    rng = np.random.default_rng(17)
    n = 4
    try:
        real = o.keygen_secret(11)
        for kind in ("one", "minus_one", "tail"):
            sk = real if kind == "tail" else co.const_secret_key(o.moduli, N, kind)
            g.set_secret_key(sk)
            for L in levels:
                mods = [int(q) for q in o.moduli[:L]]
                Q = co.prod(mods)
                phases = co.phase_batch(Q, t, N, n, seed=L)
                want = np.array([[co.bfv_round_closed_form(x, Q, t) for x in row] for row in phases], dtype=np.uint64)
                assert want[0][phases[0].index(Q - 1)] == 0
                for size in (2, 3):
                    cts = np.stack([co.bfv_ct_with_phase(row, mods, size, kind, rng, lambda ct: o.decrypt_phase(ct, sk)) for row in phases])
                    out = g.alloc(n * N)
                    g.decrypt(L, size, n, g.to_device(cts), out)
                    got = out.download((n, N))
                    for r in range(n):
                        assert np.array_equal(o.bfv_decode_phase(o.decrypt_phase(cts[r], sk)), want[r]), (kind, L, size, r)
                        assert np.array_equal(got[r], want[r]), (kind, L, size, r)
    finally:
        g.close()


# ---- CKKS decrypt --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,bits", [(2048, [60, 40, 40, 60]), (1024, [50, 45, 58])])
def test_ckks_decrypt_at_extreme_ciphertexts(be, oracle, N, bits):
    """k_dot_sk with every product at its top: ciphertexts that are all q_i - 1, all floor(q_i / 2), alternating and impulses, under the
    secret key whose every NTT value is q_i - 1 and under a real key, sizes 2 and 3, at L and L - 1"""
    g, o = _pair(be, oracle, "ckks", N, bits)
    rng = np.random.default_rng(23)
    names = eo.mixed(10, ["qm1", "half", "alt", "impulse0", "impulseN1"])
    try:
        for sk in (co.const_secret_key(o.moduli, N, "minus_one"), o.keygen_secret(11)):
            g.set_secret_key(sk)
            for L in sorted({g.L, g.L - 1}):
                for size in (2, 3):
                    cts = eo.batch(o, names, L, size, rng)
                    out = g.alloc(len(names) * L * N)
                    g.decrypt(L, size, len(names), g.to_device(cts), out)
                    got = out.download((len(names), L, N))
                    for r in range(len(names)):
                        assert np.array_equal(got[r], o.decrypt_phase(cts[r], sk)), (L, size, r, names[r])
    finally:
        g.close()


# ---- encryption ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", list(co.ENCRYPT_CHAINS))
def test_encrypt_under_the_constant_public_key(be, oracle, chain):
    """the divide-and-round by the special prime (k_divround_last_coeff, BFV; the floor_cols / floor_rows tail, CKKS) with the dropped
    residue on 0, P - 1, floor(P/2) and floor(P/2) + 1 for a third of the coefficients: device == oracle == the closed form; 35 ciphertexts,
    so the chunk of 32 is crossed with planted rows on both sides.  encrypt_zero and accumulate(count = 0) give the same ciphertexts."""
    scheme, N, bits, pb = co.ENCRYPT_CHAINS[chain]
    ckks = scheme == "ckks"
    g, o = _pair(be, oracle, scheme, N, bits, pb)
    if chain == "bfv_n16384_shoup":
        shoup.check_device("n16384_60_50_40_60_shoup", g)
    L = g.L
    pk, Cs = co.const_public_key(o.moduli, N)
    rng = np.random.default_rng(29)
    n, seed, first = 35, 0xC0FFEE1234, 1000
    try:
        g.set_public_key(pk)
        if ckks:
            plains = np.stack([o.random_poly(rng, L, 1)[0] for _ in range(n)])
            zero = np.zeros((L, N), dtype=np.uint64)
        else:
            plains = np.stack([co.bfv_edge_plain(int(o.t), N, r) for r in range(n)])
            zero = np.zeros(N, dtype=np.uint64)
        out, ez = g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
        g.encrypt(n, g.to_device(plains), seed, first, out)
        g.encrypt_zero(n, seed, first, ez)
        junk = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
        slab, tmp = g.to_device(junk), g.alloc(n * 2 * L * N)
        g.set_zero_stream(seed, first)
        g.accumulate(L, n, slab, 0, tmp)
        got, gotz, acc = out.download((n, 2, L, N)), ez.download((n, 2, L, N)), slab.download((n, 2, L, N))
        for r in range(n):
            su, s0, s1 = sn.enc_streams(first + r)
            u, e0, e1 = sn.sample_ternary(seed, su, N), sn.sample_cbd(seed, s0, N), sn.sample_cbd(seed, s1, N)
            assert np.array_equal(got[r], o.encrypt_explicit(pk, plains[r], u, e0, e1)), r
            wantz = o.encrypt_explicit(pk, zero, u, e0, e1)
            assert np.array_equal(gotz[r], wantz) and np.array_equal(acc[r], wantz), r
            if r in (0, 1, 31, 32, 34):
                want, on_edge = co.encrypt_closed_form(o, Cs, plains[r], u, e0, e1)
                assert on_edge >= 2 * N // 5
                assert np.array_equal(got[r], want), r
                assert np.array_equal(gotz[r], co.encrypt_closed_form(o, Cs, None if ckks else zero, u, e0, e1)[0]), r
    finally:
        g.close()


# ---- BFV encode / decode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["b60_40_40", "b50_40_t16", "b60x4_t31"])
def test_bfv_codec_at_the_extreme_values(be, sim, oracle, chain):
    """INT64_MIN (whose negation is itself), INT64_MAX, multiples of t and values outside (-t, t): device == host == the oracle's codec with
    the values reduced in Python; decode and decode_slots return the centred representatives"""
    N, bits, pb = co.BFV_DECRYPT_CHAINS[chain]
    g, o = _pair(be, oracle, "bfv", N, bits, pb)
    h = co.HostClient(sim, "bfv", N, bits, pb)
    t = int(o.t)
    codec = oracle.BatchCodec(N, t)
    try:
        for count in (N, len(co.bfv_extreme_values(t)), 1):
            n = 4
            x = np.stack([co.bfv_encoder_input(t, count, 3 * r) for r in range(n)])
            plain = g.alloc(n * N)
            g.bfv_encode(n, g.to_device(x.view(np.uint64)), count, plain)
            got = plain.download((n, N))
            for r in range(n):
                assert np.array_equal(got[r], h.bfv_encode(x[r])), (count, r)
                assert np.array_equal(got[r], codec.encode(np.array([int(v) % t for v in x[r]], dtype=np.int64))), (count, r)
            out = g.alloc(n * N)
            g.bfv_decode(n, plain, out)
            vals = _i64(out, (n, N))
            for r in range(n):
                assert np.array_equal(vals[r], h.bfv_decode(got[r])), (count, r)
                assert np.array_equal(vals[r, :count], co.centre_mod_t(x[r], t)) and not vals[r, count:].any(), (count, r)
            ranges = [(0, min(count, 7)), (N // 2, 3), (N - 2, 2)]
            tot = sum(c for _, c in ranges)
            outs = g.alloc(n * tot)
            g.bfv_decode_slots(n, plain, ranges, outs)
            assert np.array_equal(_i64(outs, (n, tot)), np.concatenate([vals[:, f:f + c] for f, c in ranges], axis=1)), count
    finally:
        h.close()
        g.close()


# ---- the chunk loops of the client calls ---------------------------------------------------------------------------------------------
def _chunk_rows(n, chunk):
    """row 0, the last row of the first chunk, the first of the second and the last"""
    return sorted({0, chunk - 1, chunk, n - 1})


def test_ckks_codec_across_its_chunk_boundaries(be, sim, oracle):
    """ckks_encode works in chunks of 256 vectors and ckks_decode in chunks of 128: with distinct rows a wrong `off * stride` of either loop
    shows in the first row of the second chunk"""
    N, bits, scale = 1024, co.CKKS_ENCODE_CHAIN, 2.0 ** 40
    g, o = _pair(be, oracle, "ckks", N, bits)
    h = co.HostClient(sim, "ckks", N, bits)
    try:
        L, half, n = g.L, N // 2, 257
        x = np.random.default_rng(31).uniform(-1, 1, (n, half))
        plain = g.alloc(n * L * N)
        g.ckks_encode(n, g.to_device(x.view(np.uint64)), half, scale, plain)
        got = plain.download((n, L, N))
        for r in _chunk_rows(n, 256):
            assert np.array_equal(got[r], h.ckks_encode(x[r], scale)), r
        nd = 129
        for Ld in (L, L - 1):
            sub = np.ascontiguousarray(got[:nd, :Ld])
            dpl = g.to_device(sub)
            out = g.alloc(nd * half)
            g.ckks_decode(Ld, nd, dpl, scale, out)
            vals = _f64(out, (nd, half))
            for r in _chunk_rows(nd, 128):
                assert np.array_equal(vals[r], h.ckks_decode(sub[r], scale)), (Ld, r)
            assert np.allclose(vals, x[:nd], atol=1e-6)  # every row is its own vector
            ranges = [(1, 4), (half - 3, 3)]
            outs = g.alloc(nd * 7)
            g.ckks_decode_slots(Ld, nd, dpl, scale, ranges, outs)
            assert np.array_equal(_f64(outs, (nd, 7)), np.concatenate([vals[:, f:f + c] for f, c in ranges], axis=1)), Ld
    finally:
        h.close()
        g.close()


def test_bfv_decrypt_and_decode_across_their_chunk_boundaries(be, sim, oracle):
    """BFV decrypt works in chunks of 64 ciphertexts and bfv_decode in chunks of 1024 plaintexts"""
    N, bits, pb = co.BFV_DECRYPT_CHAINS["b60_40_40"]
    g, o = _pair(be, oracle, "bfv", N, bits, pb)
    h = co.HostClient(sim, "bfv", N, bits, pb)
    rng = np.random.default_rng(37)
    t = int(o.t)
    try:
        L, n = g.L, 65
        sk = o.keygen_secret(11)
        g.set_secret_key(sk)
        for size in (2, 3):
            cts = np.stack([o.random_poly(rng, L, size) for _ in range(n)])
            out = g.alloc(n * N)
            g.decrypt(L, size, n, g.to_device(cts), out)
            got = out.download((n, N))
            for r in _chunk_rows(n, 64):
                assert np.array_equal(got[r], o.bfv_decode_phase(o.decrypt_phase(cts[r], sk))), (size, r)
        n = 1025
        plain = rng.integers(0, t, (n, N), dtype=np.uint64)
        dpl = g.to_device(plain)
        out = g.alloc(n * N)
        g.bfv_decode(n, dpl, out)
        vals = _i64(out, (n, N))
        for r in _chunk_rows(n, 1024):
            assert np.array_equal(vals[r], h.bfv_decode(plain[r])), r
        ranges = [(0, 2), (N - 1, 1)]
        outs = g.alloc(n * 3)
        g.bfv_decode_slots(n, dpl, ranges, outs)
        assert np.array_equal(_i64(outs, (n, 3)), np.concatenate([vals[:, f:f + c] for f, c in ranges], axis=1))
    finally:
        h.close()
        g.close()
