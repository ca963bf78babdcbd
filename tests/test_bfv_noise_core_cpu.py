"""The product's BFV invariant noise budget on the CPU, exact against Python integers (tests/bfv_noise_model.py), in both forms of the u64
engine (tests/csim/sim_bfv_noise.cpp compiles csrc/bfv_noise_core.h -- the function the HIP kernel k_bfv_noise_bits<W>
compiles -- and the host client):

* bfv_noise_bits<W> for every level of five chains (W = 3..18): uniform residues, and engineered coefficients whose composed value is
  0, 1, q_L - 1, the values around the centring threshold and around every word boundary of the bit-length code;
* Client::invariant_noise_budget on ciphertexts the oracle makes with the client's keys: fresh, multiplied (size 3), relinearized,
  rotated, switched down to L = 1;
* the library without a device: the entry exists, fails with HE355_E_DEVICE, and refuses a CKKS context.
No GPU."""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest

import bfv_noise_model as model
import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the five CHAINS of tests/test_bfv_level_core_cpu.py: (N, key-level bit sizes, plain bits, runs in the fold form too)
CHAINS = [
    (1024, [50, 40, 50], 20, False),
    (1024, [60, 40, 60], 20, True),
    (1024, [60, 40, 40, 60], 20, True),
    (1024, [60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 59, 60], 20, False),  # 16 data primes, both engines, any order
    (1024, [60, 40, 60, 46, 60, 40, 60, 44, 60, 40, 60, 46, 60, 42, 60, 40, 60], 20, True),   # 16 data primes a fold context holds
]
# the four chains of the issue's table, with what the reference model gave there for a fresh ciphertext: (noise_bits, budget, bits(q_L))
CLIENT_CHAINS = [
    (1024, [50, 40, 50], 20, False),
    (4096, [60, 40, 60], 20, True),
    (8192, [60, 40, 40, 60], 20, True),
    (1024, CHAINS[3][1], 20, False),
]
IDS = lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v)


@pytest.fixture(scope="module")
def sims():
    out = []
    vp, u64p, i32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    for fold in (False, True):
        L = csim_lib.load(fold)
        L.sim_bfvn_create.restype = vp
        L.sim_bfvn_create.argtypes = [C.c_size_t, i32p, C.c_size_t, C.c_int, C.c_uint64]
        L.sim_bfvn_destroy.argtypes = [vp]
        L.sim_bfvn_levels.restype = C.c_size_t
        L.sim_bfvn_levels.argtypes = [vp]
        L.sim_bfvn_q.restype = C.c_uint64
        L.sim_bfvn_q.argtypes = [vp, C.c_size_t]
        L.sim_bfvn_t.restype = C.c_uint64
        L.sim_bfvn_t.argtypes = [vp]
        L.sim_bfvn_qbits.argtypes = [vp, C.c_int]
        L.sim_bfvn_bits.argtypes = [vp, C.c_int, u64p, u64p, i32p, i32p, C.c_size_t]
        L.sim_bfvn_secret_key.argtypes = [vp, u64p]
        L.sim_bfvn_public_key.argtypes = [vp, u64p]
        L.sim_bfvn_relin_key.argtypes = [vp, u64p]
        L.sim_bfvn_galois_key.argtypes = [vp, C.c_uint32, u64p]
        L.sim_bfvn_client_budget.argtypes = [vp, u64p, C.c_size_t, C.c_size_t, i32p]
        out.append(L)
    assert [L.sim_bfvn_form() for L in out] == [0, 1]
    return out


def contexts(sims, N, bits, pb, fold_too):
    """(form, library, handle) for every form of the u64 engine a context of this chain can run"""
    arr = (C.c_int * len(bits))(*bits)
    got = []
    for form, L in enumerate(sims):
        h = L.sim_bfvn_create(N, arr, len(bits), pb, 42)
        if form == 0:
            assert h, "the Shoup form takes every chain"
        else:
            assert bool(h) == fold_too, (bits, "fold form")
        if h:
            got.append((form, L, h))
    return got


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


@pytest.mark.parametrize("N,bits,pb,fold_too", CHAINS, ids=IDS)
def test_noise_bits_every_level(sims, N, bits, pb, fold_too):
    rng = random.Random(len(bits) * 1000 + bits[1])
    ran = 0
    for form, S, h in contexts(sims, N, bits, pb, fold_too):
        Ltop, t = S.sim_bfvn_levels(h), S.sim_bfvn_t(h)
        qs = [S.sim_bfvn_q(h, i) for i in range(Ltop)]
        assert Ltop == len(bits) - 1
        for L in range(1, Ltop + 1):
            q = qs[:L]
            qL = model.q_product(q)
            assert S.sim_bfvn_qbits(h, L) == qL.bit_length()
            # (composed value wanted, residues of the phase): the engineered values, then uniform residues
            cases = [(x, model.residues_for(x, q, t)) for x in model.edge_values(qL)]
            assert len(cases) == 6 + 3 * (len(range(64, qL.bit_length() - 1, 64)) + 1)
            for _ in range(400):
                r = [rng.randrange(m) for m in q]
                x = int(model.compose(np.array([[(v * t) % m] for v, m in zip(r, q)], dtype=object), q)[0])
                cases.append((x, r))
            want_bits = [model.magnitude_bits(x, qL) for x, _ in cases]
            want_budget = [max(0, qL.bit_length() - b - 1) for b in want_bits]
            # the phase arrives in two parts, a + b = phase (mod q_i): the key-dependent part and c0
            b = np.array([[rng.randrange(m) for m in q] for _ in cases], dtype=np.uint64)
            ph = np.array([r for _, r in cases], dtype=np.uint64)
            a = np.array([[(int(ph[c, i]) - int(b[c, i])) % q[i] for i in range(L)] for c in range(len(cases))], dtype=np.uint64)
            n = len(cases)
            for aa, bb in ((a, b), (ph, None)):
                got_bits, got_budget = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
                assert S.sim_bfvn_bits(h, L, p64(aa), p64(bb) if bb is not None else None, p32(got_bits), p32(got_budget), n) == 0
                assert got_bits.tolist() == want_bits, (form, L)
                assert got_budget.tolist() == want_budget, (form, L)
            # the engineered values themselves: 0 -> 0 bits, 1 and q_L - 1 -> 1 bit, the threshold pair differs by the centring alone
            assert want_bits[0] == 0 and want_bits[1] == 1 and want_bits[2] == 1
            assert want_bits[3] == ((qL - 1) // 2).bit_length() == want_bits[4]
            ran += 1
        assert S.sim_bfvn_bits(h, 0, p64(a), None, p32(got_bits), p32(got_budget), 1) == 1
        assert S.sim_bfvn_bits(h, Ltop + 1, p64(a), None, p32(got_bits), p32(got_budget), 1) == 1
        S.sim_bfvn_destroy(h)
    assert ran == (2 if fold_too else 1) * (len(bits) - 1)


@pytest.mark.parametrize("N,bits,pb,fold_too", CLIENT_CHAINS, ids=IDS)
def test_client_budget_on_oracle_ciphertexts(sims, oracle, N, bits, pb, fold_too):
    """Client::invariant_noise_budget (host NTT, Horner with the client's own secret key, bfv_noise_bits<W>) against the model on ciphertexts
    the ORACLE's evaluator makes with the client's keys"""
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    K, Ltop, t = o.K, o.L, o.t
    rng = np.random.default_rng(N + len(bits))
    for form, S, h in contexts(sims, N, bits, pb, fold_too):
        assert [S.sim_bfvn_q(h, i) for i in range(Ltop)] == o.moduli[:Ltop] and S.sim_bfvn_t(h) == t
        sk, pk = np.empty((K, N), dtype=np.uint64), np.empty((2, K, N), dtype=np.uint64)
        rk, gk = np.empty((Ltop, 2, K, N), dtype=np.uint64), np.empty((Ltop, 2, K, N), dtype=np.uint64)
        S.sim_bfvn_secret_key(h, p64(sk))
        S.sim_bfvn_public_key(h, p64(pk))
        S.sim_bfvn_relin_key(h, p64(rk))
        elt = o.galois_elt(1)
        S.sim_bfvn_galois_key(h, elt, p64(gk))

        seen = {}

        def check(tag, ct):
            ct = np.ascontiguousarray(ct)
            size, L, _ = ct.shape
            want_bits, want_budget, qbits = model.noise_of(o, ct, sk)
            nb = C.c_int(-7)
            got = S.sim_bfvn_client_budget(h, p64(ct), size, L, C.byref(nb))
            assert (nb.value, got) == (want_bits, want_budget), (form, tag, L, qbits)
            assert S.sim_bfvn_client_budget(h, p64(ct), size, L, None) == want_budget  # the bits are optional
            seen[tag] = (want_bits, want_budget)

        x = o.encrypt(pk, rng.integers(0, t, N).astype(np.uint64), 3)
        y = o.encrypt(pk, rng.integers(0, t, N).astype(np.uint64), 4)
        check("fresh", x)
        c3 = o.bfv_multiply(x, y)
        check("multiply", c3)
        c2 = o.relinearize(c3, rk)
        check("relinearize", c2)
        check("rotate", o.rotate(c2, 1, {elt: gk}))
        low = c2
        while low.shape[1] > 1:
            low = o.mod_switch_coeff(low)
            check(f"switch{low.shape[1]}", low)
        low3 = c3
        while low3.shape[1] > 1:
            low3 = o.mod_switch_coeff(low3)
        check("switch1_size3", low3)
        # sanity of the scenario itself: a fresh ciphertext has most of its budget, a product has less, and switching never gains budget
        assert seen["fresh"][1] > seen["multiply"][1] and seen["fresh"][0] < seen["multiply"][0]
        assert seen["switch1"][1] <= seen["relinearize"][1]
        # refusals: size, level
        assert S.sim_bfvn_client_budget(h, p64(x), 1, Ltop, None) == -1 and S.sim_bfvn_client_budget(h, p64(x), 4, Ltop, None) == -1
        assert S.sim_bfvn_client_budget(h, p64(x), 2, 0, None) == -1 and S.sim_bfvn_client_budget(h, p64(x), 2, Ltop + 1, None) == -1
        S.sim_bfvn_destroy(h)


# ---- the library without a device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


NEW = "he355_bfv_noise_budget"


def test_symbol_exported_and_declared(be):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    assert hasattr(lib, NEW)
    assert NEW in be.C_ABI_SYMBOLS and (NEW + "(") in hdr
    assert hasattr(be.Context, "bfv_noise_budget")


def call(be, ctx, buf, out):
    """the entry on a context, host arrays standing in for device memory (it may not touch them)"""
    return be.lib().he355_bfv_noise_budget(ctx.h, ctx.L, 2, 1, buf.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out[1:].ctypes.data_as(C.c_void_p))


def test_no_device_no_result(be):
    """a context that was never given a device: HE355_E_DEVICE, and nothing written"""
    ctx = be.Context(be.SCHEME_BFV, 4096, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    buf, out = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64), np.full(2, -7, dtype=np.int32)
    assert call(be, ctx, buf, out) == be.E_DEVICE
    assert (buf == 0xABCD).all() and (out == -7).all()
    assert b"no CPU fallback" in be.lib().he355_last_error()
    ctx.close()


def test_ckks_context_is_refused(be):
    ctx = be.Context(be.SCHEME_CKKS, 4096, bit_sizes=[60, 40, 40, 60], sec128=False)
    buf, out = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64), np.full(2, -7, dtype=np.int32)
    assert call(be, ctx, buf, out) == be.E_INVALID_ARGS
    assert (buf == 0xABCD).all() and (out == -7).all()
    assert b"BFV context" in be.lib().he355_last_error()
    ctx.close()
