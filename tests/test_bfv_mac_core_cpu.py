"""The arithmetic of the NTT-form BFV plaintext inner product on the CPU (tests/csim/sim_bfv_mac.cpp runs csrc/bfv_mac_core.h --
the 128-bit multiply-add, the run-length rule, the reduction and the loop that cuts a sum into runs, the functions the HIP kernel
k_bfv_plain_mac compiles -- with the Barrett constants the product builds) against Python integers:

* sum_k a_k b_k mod q for chains with 60-, 50-, 45- and 40-bit primes, inner in {1, 2, run - 1, run, run + 1, 3 run + 5} with `run` the
  rule's own value for the prime, operands all q - 1, all 0 and uniform; with all q - 1 and inner = run the 128-bit sum reaches its
  largest value, and the simulator reports that it never wrapped;
* the run-length rule: floor(2^128 / (q - 1)^2) capped to kBfvMacMaxRun, for every prime of tests/golden/primes.json' chains;
* the library without a device: the five entry points exist, fail with HE355_E_DEVICE on a BFV context, and refuse a CKKS context with
  HE355_E_INVALID_ARGS -- on the host, before any device is asked for.
No GPU."""
import ctypes as C
import importlib
import json
import os

import numpy as np
import pytest

import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# key-level bit sizes: between them primes of 60, 50, 45 and 40 bits (and a few others), owned by both engines
CHAINS = [
    [60, 40, 60],
    [60, 45, 60],
    [50, 40, 50],
    [60, 50, 45, 40, 55, 59, 60],
]
N = 1024
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def sim():
    L = csim_lib.load()  # (the Shoup library: the arithmetic does not depend on the form)
    L.sim_bfvmac_create.restype = C.c_void_p
    L.sim_bfvmac_create.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int]
    L.sim_bfvmac_destroy.argtypes = [C.c_void_p]
    L.sim_bfvmac_primes.restype = C.c_size_t
    L.sim_bfvmac_primes.argtypes = [C.c_void_p]
    L.sim_bfvmac_q.restype = C.c_uint64
    L.sim_bfvmac_q.argtypes = [C.c_void_p, C.c_size_t]
    L.sim_bfvmac_run.restype = C.c_uint64
    L.sim_bfvmac_run.argtypes = [C.c_uint64]
    L.sim_bfvmac_max_run.restype = C.c_uint64
    L.sim_bfvmac_dot.argtypes = [C.c_void_p, C.c_size_t, u64p, u64p, C.c_uint64, C.c_size_t, C.c_uint64, u64p, u64p]
    return L


def p64(a):
    return a.ctypes.data_as(u64p)


def rule(q, cap):
    return min((1 << 128) // ((q - 1) ** 2), cap)


def exact_dot(a, b, q):
    """sum_k a[k][c] b[k][c] mod q in Python integers; a, b [inner][n] uint64"""
    lo = np.uint64(0xFFFFFFFF)
    a0, a1, b0, b1 = (a & lo).astype(object), (a >> np.uint64(32)).astype(object), (b & lo).astype(object), (b >> np.uint64(32)).astype(object)
    s = (a1 * b1).sum(axis=0) * (1 << 64) + ((a1 * b0).sum(axis=0) + (a0 * b1).sum(axis=0)) * (1 << 32) + (a0 * b0).sum(axis=0)
    return [int(v) % q for v in np.atleast_1d(s)]


@pytest.mark.parametrize("bits", CHAINS, ids=lambda v: "-".join(map(str, v)))
def test_simulator_equals_python_integers(sim, bits):
    arr = (C.c_int * len(bits))(*bits)
    h = sim.sim_bfvmac_create(N, arr, len(bits), 20)
    assert h
    cap = sim.sim_bfvmac_max_run()
    rng = np.random.default_rng(sum(bits) * 31 + len(bits))
    n = 3  # coefficients per case
    seen_bits = set()
    for i in range(sim.sim_bfvmac_primes(h)):
        q = sim.sim_bfvmac_q(h, i)
        assert q.bit_length() == bits[i]
        seen_bits.add(bits[i])
        run = sim.sim_bfvmac_run(q)
        assert run == rule(q, cap) and run >= 2
        for inner in (1, 2, run - 1, run, run + 1, 3 * run + 5):
            for kind in ("max", "zero", "uniform"):
                if kind == "max":
                    a = np.full((inner, n), q - 1, dtype=np.uint64)
                    b = a.copy()
                elif kind == "zero":
                    a = np.zeros((inner, n), dtype=np.uint64)
                    b = rng.integers(0, q, size=(inner, n), dtype=np.uint64)
                else:
                    a = rng.integers(0, q, size=(inner, n), dtype=np.uint64)
                    b = rng.integers(0, q, size=(inner, n), dtype=np.uint64)
                got = np.empty(n, dtype=np.uint64)
                peak = np.zeros(2, dtype=np.uint64)
                assert sim.sim_bfvmac_dot(h, i, p64(a), p64(b), inner, n, 0, p64(got), p64(peak)) == 0, (q, inner, kind)
                want = [inner * (q - 1) ** 2 % q] * n if kind == "max" else [0] * n if kind == "zero" else exact_dot(a, b, q)
                assert got.tolist() == want, (q, inner, kind)
                top = int(peak[0]) | (int(peak[1]) << 64)
                if kind == "max":  # the largest sum a run can hold: `run` terms of (q - 1)^2 (fewer if the sum is shorter)
                    assert top == min(inner, run) * (q - 1) ** 2 < (1 << 128), (q, inner)
    assert seen_bits == set(bits)
    sim.sim_bfvmac_destroy(h)


def test_sixty_bit_primes_take_256_terms_and_fill_the_accumulator(sim):
    """the figure the kernel's comment states: 256 terms under a 60-bit prime, and a full run leaves less than one term of room"""
    arr = (C.c_int * 3)(60, 40, 60)
    h = sim.sim_bfvmac_create(N, arr, 3, 20)
    q = sim.sim_bfvmac_q(h, 0)
    assert q.bit_length() == 60 and sim.sim_bfvmac_run(q) == 256
    assert 256 * (q - 1) ** 2 < (1 << 128) <= 257 * (q - 1) ** 2
    # a run one term too long is caught by the simulator's own watch (the check the peak assertions above rely on)
    a = np.full((257, 1), q - 1, dtype=np.uint64)
    got, peak = np.empty(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert sim.sim_bfvmac_dot(h, 0, p64(a), p64(a), 257, 1, 257, p64(got), p64(peak)) == 3
    sim.sim_bfvmac_destroy(h)


def test_a_sum_does_not_depend_on_where_the_runs_are_cut(sim):
    arr = (C.c_int * 3)(60, 40, 60)
    h = sim.sim_bfvmac_create(N, arr, 3, 20)
    rng = np.random.default_rng(5)
    for i in range(3):
        q = sim.sim_bfvmac_q(h, i)
        a = rng.integers(0, q, size=(700, 4), dtype=np.uint64)
        b = rng.integers(0, q, size=(700, 4), dtype=np.uint64)
        want = exact_dot(a, b, q)
        for run in (2, 3, 7, 64, 255, 256):
            got = np.empty(4, dtype=np.uint64)
            assert sim.sim_bfvmac_dot(h, i, p64(a), p64(b), 700, 4, run, p64(got), None) == 0
            assert got.tolist() == want, (q, run)
    sim.sim_bfvmac_destroy(h)


def test_run_length_rule_for_every_golden_prime(sim):
    gold = json.load(open(os.path.join(HERE, "golden", "primes.json")))
    cap = sim.sim_bfvmac_max_run()
    assert cap == 1 << 16
    primes = sorted({int(p, 16) for ch in gold["chains"] for p in ch["primes"]})
    assert len(primes) >= 6
    for q in primes:
        run = sim.sim_bfvmac_run(q)
        assert run == rule(q, cap), hex(q)
        assert run * (q - 1) ** 2 < (1 << 128)             # a run fits ...
        assert (run - 1) * (q - 1) ** 2 + (q - 1) < (1 << 128)  # ... and so does a later one: the carried residue and run - 1 terms
        assert run == (256 if q.bit_length() == 60 else cap), hex(q)


# ---- the library without a device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


NEW = ["he355_bfv_transform_to_ntt", "he355_bfv_transform_from_ntt", "he355_bfv_plain_to_ntt", "he355_bfv_multiply_plain_ntt",
       "he355_bfv_multiply_plain_accumulate"]


def call_all(be, ctx, buf, other):
    """every new entry point on a context, with host arrays standing in for device memory (none may touch them)"""
    L = be.lib()
    p, o = buf.ctypes.data_as(C.c_void_p), other.ctypes.data_as(C.c_void_p)
    ix = be.Context.pairwise()
    return [L.he355_bfv_transform_to_ntt(ctx.h, ctx.L, 2, 1, p, p),
            L.he355_bfv_transform_from_ntt(ctx.h, ctx.L, 2, 1, p, p),
            L.he355_bfv_plain_to_ntt(ctx.h, ctx.L, 1, p, o),
            L.he355_bfv_multiply_plain_ntt(ctx.h, ctx.L, 2, 1, p, o, ix, p),
            L.he355_bfv_multiply_plain_accumulate(ctx.h, ctx.L, 2, 1, 1, 1, p, 1, 1, p, 1, 1, o)]


def test_symbols_exported_and_declared(be):
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
        assert hasattr(be.Context, s[len("he355_"):])
    assert "[UPSTREAM-UNVERIFIED]" in hdr and "does not track which form" in hdr


def test_no_device_no_result(be):
    ctx = be.Context(be.SCHEME_BFV, 4096, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)
    buf = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    other = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    assert call_all(be, ctx, buf, other) == [be.E_DEVICE] * 5
    assert (buf == 0xABCD).all() and (other == 0xABCD).all()
    assert b"no CPU fallback" in be.lib().he355_last_error()
    ctx.close()


def test_ckks_context_is_refused_on_the_host(be):
    ctx = be.Context(be.SCHEME_CKKS, 4096, bit_sizes=[60, 40, 40, 60], sec128=False)
    buf = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    other = np.full(2 * ctx.L * 4096, 0xABCD, dtype=np.uint64)
    assert call_all(be, ctx, buf, other) == [be.E_INVALID_ARGS] * 5
    assert (buf == 0xABCD).all() and (other == 0xABCD).all()
    assert b"BFV context" in be.lib().he355_last_error()
    ctx.close()
