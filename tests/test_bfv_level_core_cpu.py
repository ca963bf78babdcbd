"""The product's per-coefficient BFV level arithmetic on the CPU (tests/csim/sim_bfv_level.cpp runs csrc/bfv_level_core.h -- the
functions the HIP kernels k_bfv_mod_switch, k_bfv_addsub_plain and k_bfv_lift_plain compile -- on the tables the product uploads)
against Python integers and the oracle, in both forms of the u64 engine:

* the drop chain (BFV mod_switch_to: repeated divide-and-round by the last prime), every (L, L_to), random coefficients and the
  edges (0, q - 1, values where c_last + floor(q_last / 2) wraps), equal to repeated oracle.mod_switch_coeff;
* Delta_L(m) = floor((q_L m + floor((t + 1) / 2)) / t) mod q_i for every L, and at the top level equal to c0 of an oracle encryption
  with zero randomness;
* the centred lift of multiply_plain;
* the library without a device: the four entry points exist, fail with HE355_E_DEVICE, and refuse a CKKS context.
No GPU."""
import ctypes as C
import importlib
import os
import random

import numpy as np
import pytest

import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (N, key-level bit sizes, plain bits, runs in the fold form too)
CHAINS = [
    (1024, [50, 40, 50], 20, False),
    (1024, [60, 40, 60], 20, True),
    (1024, [60, 40, 40, 60], 20, True),
    (1024, [60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 59, 60], 20, False),  # 16 data primes, both engines, any order
    (1024, [60, 40, 60, 46, 60, 40, 60, 44, 60, 40, 60, 46, 60, 42, 60, 40, 60], 20, True),   # 16 data primes a fold context holds
]


@pytest.fixture(scope="module")
def sims():
    out = []
    u64p = C.POINTER(C.c_uint64)
    for fold in (False, True):
        L = csim_lib.load(fold)
        L.sim_bfvl_create.restype = C.c_void_p
        L.sim_bfvl_create.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int]
        L.sim_bfvl_destroy.argtypes = [C.c_void_p]
        L.sim_bfvl_levels.restype = C.c_size_t
        L.sim_bfvl_levels.argtypes = [C.c_void_p]
        L.sim_bfvl_q.restype = C.c_uint64
        L.sim_bfvl_q.argtypes = [C.c_void_p, C.c_size_t]
        L.sim_bfvl_t.restype = C.c_uint64
        L.sim_bfvl_t.argtypes = [C.c_void_p]
        L.sim_bfvl_f64.argtypes = [C.c_void_p, C.c_size_t]
        L.sim_bfvl_drop.argtypes = [C.c_void_p, C.c_int, C.c_int, u64p, u64p, C.c_size_t]
        L.sim_bfvl_delta.argtypes = [C.c_void_p, C.c_int, u64p, u64p, C.c_size_t]
        L.sim_bfvl_lift.argtypes = [C.c_void_p, C.c_int, u64p, u64p, C.c_size_t]
        out.append(L)
    assert [L.sim_bfvl_form() for L in out] == [0, 1]
    return out


def contexts(sims, N, bits, pb, fold_too):
    """(form, library, handle) for every form of the u64 engine a context of this chain can run"""
    arr = (C.c_int * len(bits))(*bits)
    got = []
    for form, L in enumerate(sims):
        h = L.sim_bfvl_create(N, arr, len(bits), pb)
        if form == 0:
            assert h, "the Shoup form takes every chain"
        else:
            assert bool(h) == fold_too, (bits, "fold form")
        if h:
            got.append((form, L, h))
    return got


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def drop_once(x, qs):
    """one divide_and_round_q_last step on Python integers: residues under qs -> residues under qs[:-1]"""
    last, half = qs[-1], qs[-1] // 2
    r = (x[-1] + half) % last
    return [((x[i] - (r % qs[i] - half % qs[i])) * pow(last, -1, qs[i])) % qs[i] for i in range(len(qs) - 1)]


def coefficient_vectors(rng, qs, n):
    """n residue vectors under qs: the edges of every prime first, then uniform ones"""
    vecs = []
    edge = lambda q: [0, 1, q - 1, q - 2, q // 2, q - q // 2 - 1, q - q // 2, q - q // 2 + 1, q // 2 - 1, q // 2 + 1]
    for k in range(10):
        vecs.append([edge(q)[k] for q in qs])
    for _ in range(60):  # edges of the dropped primes against anything below them
        vecs.append([rng.choice(edge(q)) if rng.random() < 0.5 else rng.randrange(q) for q in qs])
    while len(vecs) < n:
        vecs.append([rng.randrange(q) for q in qs])
    return vecs[:n]


@pytest.mark.parametrize("N,bits,pb,fold_too", CHAINS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_drop_chain_every_level_pair(sims, oracle, N, bits, pb, fold_too):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    rng = random.Random(len(bits) * 1000 + bits[1])
    ran = 0
    for form, S, h in contexts(sims, N, bits, pb, fold_too):
        Ltop = S.sim_bfvl_levels(h)
        qs = [S.sim_bfvl_q(h, i) for i in range(Ltop)]
        assert Ltop == o.L == len(bits) - 1 and qs == o.moduli[:Ltop]
        for L in range(1, Ltop + 1):
            vecs = coefficient_vectors(rng, qs[:L], N)
            x = np.array(vecs, dtype=np.uint64)              # [N][L]
            ct = np.ascontiguousarray(x.T)[None]             # [1][L][N] for the oracle
            want_py, want_or = vecs, ct
            for L_to in range(L, 0, -1):
                if L_to < L:
                    want_py = [drop_once(v, qs[:L_to + 1]) for v in want_py]
                    want_or = o.mod_switch_coeff(want_or)
                got = np.empty((N, L_to), dtype=np.uint64)
                assert S.sim_bfvl_drop(h, L, L_to, p64(x), p64(got), N) == 0
                assert got.tolist() == want_py, (form, L, L_to)
                assert np.array_equal(got.T, want_or[0]), (form, L, L_to)
                ran += 1
        assert S.sim_bfvl_drop(h, L, 0, p64(x), p64(got), 1) == 1 and S.sim_bfvl_drop(h, 1, 2, p64(x), p64(got), 1) == 1
        S.sim_bfvl_destroy(h)
    Ltop = len(bits) - 1
    assert ran == (2 if fold_too else 1) * Ltop * (Ltop + 1) // 2


def plain_values(rng, t, n):
    vals = [0, 1, t // 2, (t + 1) // 2, t - 1, 2, t - 2, t // 2 - 1, (t + 1) // 2 + 1]
    while len(vals) < n:
        vals.append(rng.randrange(t))
    return vals[:n]


@pytest.mark.parametrize("N,bits,pb,fold_too", CHAINS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_delta_and_lift(sims, oracle, N, bits, pb, fold_too):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    rng = random.Random(77 + len(bits))
    sk = o.keygen_secret(3)
    pk = o.keygen_public(sk, 4)
    zero = np.zeros(N, dtype=np.int32)
    for form, S, h in contexts(sims, N, bits, pb, fold_too):
        Ltop, t = S.sim_bfvl_levels(h), S.sim_bfvl_t(h)
        qs = [S.sim_bfvl_q(h, i) for i in range(Ltop)]
        assert t == o.t
        m = plain_values(rng, t, N)
        ma = np.array(m, dtype=np.uint64)
        for L in range(1, Ltop + 1):
            qL = 1
            for q in qs[:L]:
                qL *= q
            got = np.empty((N, L), dtype=np.uint64)
            assert S.sim_bfvl_delta(h, L, p64(ma), p64(got), N) == 0
            want = [[((qL * v + (t + 1) // 2) // t) % q for q in qs[:L]] for v in m]
            assert got.tolist() == want, (form, L)
            if L == Ltop:  # an encryption with u = e0 = e1 = 0 is (Delta(m), 0)
                ct = o.encrypt_explicit(pk, ma, zero, zero, zero)
                assert not ct[1].any()
                assert np.array_equal(got.T, ct[0]), form
            lift = np.empty((N, L), dtype=np.uint64)
            assert S.sim_bfvl_lift(h, L, p64(ma), p64(lift), N) == 0
            assert lift.tolist() == [[(v if v < (t + 1) // 2 else v - t) % q for q in qs[:L]] for v in m], (form, L)
        S.sim_bfvl_destroy(h)


# ---- the library without a device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


NEW = ["he355_bfv_mod_switch", "he355_bfv_add_plain", "he355_bfv_sub_plain", "he355_bfv_multiply_plain"]


def call_all(be, ctx, buf):
    """every new entry point on a context, with a host array standing in for device memory (none may touch it)"""
    L = be.lib()
    p = buf.ctypes.data_as(C.c_void_p)
    ix = be.Context.pairwise()
    return [L.he355_bfv_mod_switch(ctx.h, ctx.L, 1, 2, 1, p, p),
            L.he355_bfv_add_plain(ctx.h, ctx.L, 2, 1, p, p, ix, p),
            L.he355_bfv_sub_plain(ctx.h, ctx.L, 2, 1, p, p, ix, p),
            L.he355_bfv_multiply_plain(ctx.h, ctx.L, 2, 1, p, p, ix, p)]


def test_symbols_exported_and_declared(be):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr


def test_no_device_no_result(be):
    """a context that was never given a device: HE355_E_DEVICE from every new entry point, and nothing written"""
    ctx = be.Context(be.SCHEME_BFV, 4096, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    buf = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    assert call_all(be, ctx, buf) == [be.E_DEVICE] * 4
    assert (buf == 0xABCD).all()
    assert b"no CPU fallback" in be.lib().he355_last_error()
    ctx.close()


def test_ckks_context_is_refused(be):
    ctx = be.Context(be.SCHEME_CKKS, 4096, bit_sizes=[60, 40, 40, 60], sec128=False)
    buf = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    assert call_all(be, ctx, buf) == [be.E_INVALID_ARGS] * 4
    assert (buf == 0xABCD).all()
    assert b"BFV context" in be.lib().he355_last_error()
    ctx.close()
