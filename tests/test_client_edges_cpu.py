"""The client half (encoders, encryptor, decryptor) at structured and extreme operands, on the CPU: the product's host client (tests/csim,
the same inline code the device kernels compile) against references that share nothing with it -- the mpmath fixture
tests/golden/client_edge_vectors.json for the CKKS codec, Python-integer closed forms for the BFV rounding and for encryption under a
constant public key (tests/client_operands.py).  tests/test_gpu_client_edges.py holds the device to the host and to the same references.

The figures these tests print (pytest -s) are the CPU table of profiles/client_edges.txt."""
import numpy as np
import pytest

import client_operands as co
import sampler_np as sn


@pytest.fixture(scope="module")
def sim():
    return co.host_sim()


@pytest.fixture(scope="module")
def fixture():
    return co.load_fixture()


def test_fixture_is_within_the_size_of_the_largest_fixture_and_covers_the_case_list(fixture):
    import os
    golden = os.path.dirname(co.FIXTURE)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f.endswith(".json") and f != os.path.basename(co.FIXTURE)]
    assert os.path.getsize(co.FIXTURE) <= max(others)
    enc = {c["id"] for c in fixture["encode"]}
    assert enc == {f"{name}/N{N}/s{s}" for name in co.CKKS_INPUTS for N in co.CKKS_ENCODE_N for s in (30, 40, 45)}
    dec = {c["id"] for c in fixture["decode"]}
    want = {f"{ch}/L{L}/{fam}/{s}" for ch, (_, _, levels) in co.DECODE_CHAINS.items() for L in levels for fam in co.DECODE_FAMILIES for s in co.DECODE_SCALES[fam]}
    assert dec == want
    assert {s for fam in co.DECODE_FAMILIES for s in co.DECODE_SCALES[fam]} == {"2^30", "2^90", "Q"}
    for c in fixture["encode"]:  # the reference's own error: the final rounding alone leaves up to 1/2 (exactly representable inputs: 0)
        assert c["tie_share"] <= co.TIE_SHARE_CAP
        assert float.fromhex(c["E_np"]) < 4.0


@pytest.mark.parametrize("N", co.CKKS_ENCODE_N)
def test_host_ckks_encode_against_the_exact_coefficients(sim, oracle, fixture, N):
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=co.CKKS_ENCODE_CHAIN, sec128=False)
    h = co.HostClient(sim, "ckks", N, co.CKKS_ENCODE_CHAIN)
    try:
        for case in [c for c in fixture["encode"] if c["N"] == N]:
            values = co.ckks_input(case["input"], N)
            assert co.digest(values) == case["digest"], case["id"]
            plain = h.ckks_encode(values, float.fromhex(case["scale"]))
            coeffs = co.coeffs_from_plain(o, plain)
            for i in range(1, o.L):  # every residue row holds the same integers
                qi = int(o.moduli[i])
                assert np.array_equal(o.intt(i, plain[i]), np.array([c % qi for c in coeffs], dtype=np.uint64)), (case["id"], i)
            case = dict(case, positions=fixture["positions"][str(N)])
            f = co.check_encode_case(case, coeffs, "host")
            e_np = float.fromhex(case["E_np"])
            # the fixture keeps the exact values at 16 positions; at EVERY position codec and numpy are each within their bound of the
            # exact value, so within (2 + 1) E_np of each other
            ref = co.coeffs_from_plain(o, oracle.ckks_encode(o, values, float.fromhex(case["scale"])))
            assert max(abs(a - b) for a, b in zip(coeffs, ref)) <= (co.ENCODE_FACTOR + 1) * e_np, case["id"]
            print(f"encode {case['id']:28s} E_np {e_np:.4f} codec {f['err']:.4f} ratio {f['err'] / e_np if e_np else 0.0:.3f} "
                  f"near-tie share {case['tie_share']:.5f} tie rule {case['tie_rule']}")
    finally:
        h.close()


def test_host_ckks_encode_negative_multiple_of_a_prime(sim, oracle):
    """-k q_i is 0 under q_i (not q_i - 0) and q_j - (k q_i mod q_j) under the other primes"""
    N = 1024
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=co.CKKS_ENCODE_CHAIN, sec128=False)
    h = co.HostClient(sim, "ckks", N, co.CKKS_ENCODE_CHAIN)
    try:
        rows, picks = co.negative_prime_multiples(o)
        for row, (i, k) in zip(rows, picks):
            co.check_negative_prime_multiple(o, h.ckks_encode(row, 1.0), i, k)
    finally:
        h.close()


@pytest.mark.parametrize("chain", list(co.DECODE_CHAINS))
def test_host_ckks_decode_against_the_exact_slots(sim, oracle, fixture, chain):
    N, bits, levels = co.DECODE_CHAINS[chain]
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    h = co.HostClient(sim, "ckks", N, bits)
    try:
        for L, fam, plain, cases in co.decode_operands(o, chain, fixture):
            for case in cases:
                got = h.ckks_decode(plain, float.fromhex(case["scale"]))
                f = co.check_decode_case(case, got, "host")
                e_np = float.fromhex(case["E_np"])
                # (the fixture keeps 5 slots; at every slot: within (4 + 1) E_np of numpy, by the triangle inequality)
                ref = oracle.ckks_decode(o, plain, float.fromhex(case["scale"])).real
                assert float(np.max(np.abs(got - ref))) <= (co.DECODE_FACTOR + 1) * e_np, case["id"]
                print(f"decode {case['id']:28s} E_np {e_np:.3e} codec {f['err']:.3e} ratio {f['err'] / e_np if e_np else 0.0:.3f}")
    finally:
        h.close()


@pytest.mark.parametrize("chain", list(co.BFV_DECRYPT_CHAINS))
def test_bfv_decrypt_at_the_planted_phases(sim, oracle, chain):
    """host client == oracle == round(t x / Q) mod t in Python integers, at the tie points of the rounding and the ends of [0, Q), at every
    level of the chain, for (c0, 0) ciphertexts and for sizes 2 and 3 under the constant secret keys 1 and -1"""
    N, bits, pb = co.BFV_DECRYPT_CHAINS[chain]
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    h = co.HostClient(sim, "bfv", N, bits, pb)
    t = int(o.t)
    rng = np.random.default_rng(11)
    try:
        own = h.secret_key()
        for L in range(1, o.L + 1):
            mods = [int(q) for q in o.moduli[:L]]
            Q = co.prod(mods)
            for r, phases in enumerate(co.phase_batch(Q, t, N, 2, seed=L)):
                want = np.array([co.bfv_round_closed_form(x, Q, t) for x in phases], dtype=np.uint64)
                if r == 0:  # the planted row: the result t (x = Q - 1) wraps to 0, and both sides of a tie are present
                    assert want[phases.index(Q - 1)] == 0 and len(set(want.tolist())) > 20
                assert np.array_equal(o.bfv_decode_phase(co.to_residues(phases, mods)), want), (L, r)
                for size, kind in ((2, "zero"), (3, "zero"), (2, "one"), (3, "one"), (2, "minus_one"), (3, "minus_one")):
                    ct = co.bfv_ct_with_phase(phases, mods, size, kind, rng)
                    sk = own if kind == "zero" else co.const_secret_key(o.moduli, N, kind)
                    assert np.array_equal(o.bfv_decode_phase(o.decrypt_phase(ct, sk)), want), (L, r, size, kind)
                    assert np.array_equal(h.decrypt(ct, None if kind == "zero" else sk), want), (L, r, size, kind)
    finally:
        h.close()


@pytest.mark.parametrize("chain", ["b60_40_40", "b50_40_t16", "b60x4_t31"])
def test_bfv_codec_at_the_extreme_values(sim, oracle, chain):
    """host encoder == the oracle's BatchCodec with the values reduced mod t in Python; the decoder returns the centred representatives"""
    N, bits, pb = co.BFV_DECRYPT_CHAINS[chain]
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    h = co.HostClient(sim, "bfv", N, bits, pb)
    t = int(o.t)
    codec = oracle.BatchCodec(N, t)
    try:
        for count, shift in ((N, 0), (N, 7), (len(co.bfv_extreme_values(t)), 0), (1, 11)):
            x = co.bfv_encoder_input(t, count, shift)
            want = codec.encode(np.array([int(v) % t for v in x], dtype=np.int64))
            got = h.bfv_encode(x)
            assert np.array_equal(got, want), (count, shift)
            back = h.bfv_decode(got)
            assert np.array_equal(back[:count], co.centre_mod_t(x, t)) and not back[count:].any(), (count, shift)
            assert np.array_equal(codec.decode(got)[:count] % t, np.array([int(v) % t for v in x]))
    finally:
        h.close()


@pytest.mark.parametrize("chain", list(co.ENCRYPT_CHAINS))
def test_encryption_under_the_constant_public_key(oracle, chain):
    """oracle.encrypt_explicit == the closed form, with the dropped residue of the special prime on 0, P - 1, floor(P/2) and their
    neighbours for a large share of the coefficients (uniform u pk + e puts it there with probability ~ 0)"""
    scheme, N, bits, pb = co.ENCRYPT_CHAINS[chain]
    ckks = scheme == "ckks"
    o = oracle.Context(oracle.SCHEME_CKKS if ckks else oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    pk, Cs = co.const_public_key(o.moduli, N)
    rng = np.random.default_rng(5)
    seed, first = 0xC0FFEE1234, 1000
    for r in (0, 1, 2):
        su, s0, s1 = sn.enc_streams(first + r)
        u, e0, e1 = sn.sample_ternary(seed, su, N), sn.sample_cbd(seed, s0, N), sn.sample_cbd(seed, s1, N)
        plain = o.random_poly(rng, o.L, 1)[0] if ckks else co.bfv_edge_plain(int(o.t), N, r)
        want, on_edge = co.encrypt_closed_form(o, Cs, plain, u, e0, e1)
        assert on_edge >= 2 * N // 5, (r, on_edge)  # (measured: 640 of 2048)
        assert np.array_equal(o.encrypt_explicit(pk, plain, u, e0, e1), want), r
