"""The arithmetic of the complex scalar combination, the residue pairs and the host client's complex codec on the CPU (tests/csim/sim_cplx.cpp
runs csrc/cplx_core.h -- the functions the HIP kernel k_scalar_combine_cplx compiles --, csrc/cplx_args.h's unit and residue rule, and
client/he_client.cpp) against Python integers and the oracle, in both builds of the u64 engine:

* the combination over a window of NTT indices that crosses a sign change (bit log2 N - 2): 1, 2, 256, 257 and 513 terms under two 60-bit
  primes with every operand and both scalars q - 1 -- 257 terms under a 60-bit prime: one fold of the 128-bit sum -- and uniform ones, with
  and without a constant pair, at the prime's own run length and at forced short ones; 14- to 31-bit primes;
* the residue pairs against (A +- B u) % q with A = round(v_re), B = round(v_im / sqrt 2); refusals of either part;
* the units and the pairs as the C ABI forms them against the oracle's transform of J;
* the host codec against the mpmath fixture tests/golden/ckks_complex_vectors.json under the real codec's bounds
  (tests/test_client_edges_cpu.py): encode within ENCODE_FACTOR x E_np of the exact coefficients, im = +0.0 the real encoder's bits; the
  imaginary parts of the decode within DECODE_FACTOR x E_np_im of the exact ones, the re parts the real decoder's bits.
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import ckks_complex_operands as cx
import ckks_complex_ref as cref
import client_operands as co
import csim_lib
import oracle as ho

u64p = C.POINTER(C.c_uint64)
dp = C.POINTER(C.c_double)
Q60 = [0xfffffffffff2801, 0xffffffffffc0001]
SMALL = [12289, 65537, 786433, 8380417, 1073479681, 2147352577]  # 14 to 31 bits
TERMS = [1, 2, 256, 257, 513]


def declare(L):
    L.sim_cplx_combine.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u64p]
    L.sim_cplx_combine.restype = None
    L.sim_cplx_scalar.argtypes = [C.c_double, C.c_double, u64p, u64p, C.c_int, u64p]
    L.sim_cplx_scalar.restype = C.c_int
    L.sim_cplx_units.argtypes = [C.c_void_p, C.c_int, u64p]
    L.sim_cplx_units.restype = C.c_int
    L.sim_cplx_residues.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, u64p]
    L.sim_cplx_residues.restype = C.c_int
    L.sim_params_create.restype = C.c_void_p
    L.sim_params_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.c_int]
    L.sim_params_destroy.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def p64(a):
    return a.ctypes.data_as(u64p)


LOGN, E0, WIDTH = 10, 252, 8  # NTT indices 252 .. 259 of N = 1024: bit 8 changes at 256


def check(sim, q, x, a, cst, runs):
    terms, n = x.shape
    assert n == WIDTH
    half = [((E0 + e) >> (LOGN - 2)) & 1 for e in range(n)]
    assert half == [0, 0, 0, 0, 1, 1, 1, 1]
    want = [(sum(int(x[k, e]) * int(a[k, half[e]]) for k in range(terms)) + (int(cst[half[e]]) if cst is not None else 0)) % q for e in range(n)]
    for run in runs:
        out = np.empty(n, dtype=np.uint64)
        sim.sim_cplx_combine(n, LOGN, E0, q, terms, run, p64(np.ascontiguousarray(x)), p64(np.ascontiguousarray(a)), p64(cst) if cst is not None else None, p64(out))
        assert [int(v) for v in out] == want, (hex(q), terms, run, cst)


@pytest.mark.parametrize("q", Q60, ids=hex)
@pytest.mark.parametrize("terms", TERMS)
def test_the_combination_across_a_sign_change_at_the_edge_of_a_run(sim, q, terms):
    assert (2 ** 128 - 1) // (q - 1) ** 2 == 256  # 257 terms: one fold
    rng = np.random.default_rng(terms)
    full_x, full_a = np.full((terms, WIDTH), q - 1, dtype=np.uint64), np.full((terms, 2), q - 1, dtype=np.uint64)
    uni_x, uni_a = rng.integers(0, q, (terms, WIDTH), dtype=np.uint64), rng.integers(0, q, (terms, 2), dtype=np.uint64)
    for x, a in ((full_x, full_a), (uni_x, uni_a), (full_x, uni_a)):
        for cst in (None, np.array([q - 1, q - 1], dtype=np.uint64), np.array([0, 12345], dtype=np.uint64)):
            check(sim, q, x, a, cst, (0, 2, 3, 256))


@pytest.mark.parametrize("q", SMALL)
def test_the_combination_under_small_primes(sim, q):
    rng = np.random.default_rng(q)
    for terms in (1, 2, 257):
        x, a = rng.integers(0, q, (terms, WIDTH), dtype=np.uint64), rng.integers(0, q, (terms, 2), dtype=np.uint64)
        for cst in (None, np.array([q - 1, 1], dtype=np.uint64)):
            check(sim, q, x, a, cst, (0, 2))
            check(sim, q, np.full((terms, WIDTH), q - 1, dtype=np.uint64), np.full((terms, 2), q - 1, dtype=np.uint64), cst, (0, 5))


def test_residue_pairs_against_python_integers(sim):
    qs = np.array(Q60 + SMALL + [0xffffff7801], dtype=np.uint64)
    rng = np.random.default_rng(3)
    us = np.array([int(rng.integers(0, int(q))) for q in qs[:-1]] + [int(qs[-1]) - 1], dtype=np.uint64)  # any u < q: the rule is A +- B u
    n = len(qs)
    parts = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, math.sqrt(2.0), -math.sqrt(2.0), 2.0 * math.sqrt(2.0), 2.0 ** 40 * 0.3, -(2.0 ** 52 + 1), 2.0 ** 90, -(2.0 ** 125),
             math.nextafter(2.0 ** 126, 0.0), float(int(qs[0])), 1234567.5]
    out = np.empty(2 * n, dtype=np.uint64)
    for re in parts:
        for im in parts:
            assert sim.sim_cplx_scalar(re, im, p64(qs), p64(us), n, p64(out)) == 1, (re, im)
            a, b = int(round(re)), int(round(im / math.sqrt(2.0)))
            assert [int(v) for v in out] == [(a + b * int(u)) % int(q) for q, u in zip(qs, us)] + [(a - b * int(u)) % int(q) for q, u in zip(qs, us)], (re, im)
    for bad in (float("inf"), float("nan"), 2.0 ** 126, -(2.0 ** 126)):
        assert sim.sim_cplx_scalar(bad, 1.0, p64(qs), p64(us), n, p64(out)) == 0
    for bad in (float("inf"), float("nan"), 2.0 ** 126.5, -(2.0 ** 127)):  # (the imaginary part is divided by sqrt 2 first)
        assert sim.sim_cplx_scalar(1.0, bad, p64(qs), p64(us), n, p64(out)) == 0
    assert sim.sim_cplx_scalar(1.0, 2.0 ** 126, p64(qs), p64(us), n, p64(out)) == 1  # 2^126 / sqrt 2 < 2^126


@pytest.mark.parametrize("N", [1024, 4096])
def test_units_and_pairs_as_the_abi_forms_them(sim, N):
    bits = [60, 40, 40, 60]
    o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    p = sim.sim_params_create(2, N, (C.c_int * len(bits))(*bits), len(bits), 0, 0)
    L = o.L
    u = np.empty(L, dtype=np.uint64)
    assert sim.sim_cplx_units(p, L, p64(u)) == 1
    assert [int(v) for v in u] == cref.units(o, L)
    assert sim.sim_cplx_units(p, 0, p64(u)) == 0 and sim.sim_cplx_units(p, L + 1, p64(u)) == 0 and sim.sim_cplx_units(p, L, None) == 0
    out = np.empty(2 * L, dtype=np.uint64)
    for v in ((2.0 ** 40 * 0.25, -(2.0 ** 40) * 0.75), (-1.0, 1.0), (0.0, 2.0 ** 100)):
        assert sim.sim_cplx_residues(p, L, v[0], v[1], p64(out)) == 1
        assert out.reshape(2, L).tolist() == cref.scalar_residues(o.moduli, cref.units(o, L), L, *v)
    assert sim.sim_cplx_residues(p, L, float("nan"), 0.0, p64(out)) == 0 and sim.sim_cplx_residues(p, L, 0.0, 1.0, None) == 0
    sim.sim_params_destroy(p)


# ---- the host client's complex codec ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return cx.load_fixture()


@pytest.mark.parametrize("N", co.CKKS_ENCODE_N)
def test_host_complex_encode_against_the_exact_coefficients(oracle, fixture, N):
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=co.CKKS_ENCODE_CHAIN, sec128=False)
    h = cx.ComplexHost(co.host_sim(), N, co.CKKS_ENCODE_CHAIN)
    try:
        for case in [c for c in fixture["encode"] if c["N"] == N]:
            vals = cx.complex_input(N, case["count"])
            assert co.digest(vals.view(np.float64)) == case["digest"], case["id"]
            plain = h.ckks_encode_complex(vals, cx.SCALE)
            coeffs = co.coeffs_from_plain(o, plain)
            for i in range(1, o.L):  # every residue row holds the same integers
                qi = int(o.moduli[i])
                assert np.array_equal(o.intt(i, plain[i]), np.array([c % qi for c in coeffs], dtype=np.uint64)), (case["id"], i)
            err = cx.check_encode_case(fixture, case, coeffs, "host")
            e_np = float.fromhex(case["E_np"])
            # at EVERY position codec and numpy are each within their bound of the exact value: within (2 + 1) E_np of each other
            ref = co.coeffs_from_plain(o, oracle.ckks_encode(o, vals, cx.SCALE))
            assert max(abs(a - b) for a, b in zip(coeffs, ref)) <= (co.ENCODE_FACTOR + 1) * e_np, case["id"]
            print(f"complex encode {case['id']:18s} E_np {e_np:.4f} codec {err:.4f}")
            real = np.ascontiguousarray(vals.real)
            assert np.array_equal(h.ckks_encode_complex(real.astype(np.complex128), cx.SCALE), h.ckks_encode(real, cx.SCALE)), case["id"]  # im = +0.0
            back = h.ckks_decode_complex(plain, cx.SCALE)  # the round trip: encoder rounding (1/2 per coefficient, N of them) over the scale
            assert float(np.max(np.abs(back[:case["count"]] - vals))) <= N / cx.SCALE and float(np.max(np.abs(back[case["count"]:]), initial=0.0)) <= N / cx.SCALE
    finally:
        h.close()


@pytest.mark.parametrize("chain", list(cx.DECODE_LEVELS))
def test_host_complex_decode_against_the_exact_slots(oracle, fixture, chain):
    N, bits, _ = co.DECODE_CHAINS[chain]
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
    h = cx.ComplexHost(co.host_sim(), N, bits)
    real_fixture = co.load_fixture()
    by_id = {c["id"]: c for c in fixture["decode"]}
    try:
        for L, fam, plain, cases in co.decode_operands(o, chain, real_fixture):
            if L not in cx.DECODE_LEVELS[chain]:
                continue
            for case in cases:
                scale = float.fromhex(case["scale"])
                got = h.ckks_decode_complex(plain, scale)
                assert np.array_equal(got.real, h.ckks_decode(plain, scale)), case["id"]  # the re parts: the real decoder's bits
                co.check_decode_case(case, got.real, "host")
                im_case = by_id[case["id"]]
                assert im_case["digest"] == case["digest"]
                err = cx.check_decode_case(im_case, case["positions"], got.imag, "host")
                e_np = float.fromhex(im_case["E_np_im"])
                ref = oracle.ckks_decode(o, plain, scale).imag  # at every slot: within (4 + 1) E_np of numpy
                assert float(np.max(np.abs(got.imag - ref))) <= (co.DECODE_FACTOR + 1) * e_np, case["id"]
                print(f"complex decode {case['id']:28s} E_np_im {e_np:.3e} codec {err:.3e}")
    finally:
        h.close()
