"""The per-coefficient arithmetic of a level of the BFV selection tree on the CPU (tests/csim/sim_bfv_select.cpp runs the functions of
csrc/bfv_gadget_core.h that the HIP kernels k_bfv_select_cols_fwd, k_bfv_select_spread, k_bfv_select_cols_inv and k_bfv_select_add compile), in
both builds of the u64 engine, against Python integers:

* the DIFF digit is digit_g((odd - even) mod q_i), the plain integer below 2^v, reduced once where it is not below the output prime q_j: for
  EVERY v in 1..63, every digit g < ceil(bitlen(q_i) / v), chain primes of 40, 50 and 60 bits as the nodes' prime and as the output prime, and
  odd, even in {0, 1, q - 1, floor(q / 2)} in every pairing (odd = even, the borrow and no borrow included) plus uniform words;
* the digits put together again give (odd - even) mod q_i: the gadget identity of the difference;
* the tail's add is (product + even) mod q_i at the same operands (the wrap and no wrap);
* the library without a device: the entry point exists, is declared and bound.
No GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import csim_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    L = csim_lib.load(fold=request.param)
    L.sim_bfvsel_diff.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.sim_bfvsel_diff.restype = C.c_uint64
    L.sim_bfvsel_diff_digits.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_uint64, u64p]
    L.sim_bfvsel_diff_digits.restype = None
    L.sim_bfvsel_add.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L.sim_bfvsel_add.restype = C.c_uint64
    return L


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if not os.path.exists(mod.LIB_PATH):
        mod.build()
    return mod


@pytest.fixture(scope="module")
def primes(be):
    out = set()
    for bits in ([60, 40, 60], [50, 40, 50]):
        ctx = be.Context(be.SCHEME_BFV, 1024, bit_sizes=bits, plain_bits=20, sec128=False)
        out |= set(ctx.moduli)
        ctx.close()
    assert {q.bit_length() for q in out} == {40, 50, 60}
    return sorted(out)


def operands(q, rng):
    edge = [0, 1, q - 1, q // 2]
    pairs = [(o, e) for o in edge for e in edge]
    pairs += [(int(o), int(e)) for o, e in rng.integers(0, q, (4, 2), dtype=np.uint64)]
    return pairs


def test_diff_digit_for_every_width(sim, primes):
    rng = np.random.default_rng(31)
    buf = (C.c_uint64 * 64)()
    # one prime of each width as the nodes' prime, every prime as the output prime
    own = {q.bit_length(): q for q in primes}.values()
    for qi in own:
        ops = operands(qi, rng)
        for v in range(1, 64):
            E = -(-qi.bit_length() // v)
            for odd, even in ops:
                d = (odd - even) % qi
                assert sim.sim_bfvsel_diff(odd, even, qi) == d, (qi, odd, even)
                digits = [(d >> (g * v)) & ((1 << v) - 1) for g in range(E)]
                assert sum(x << (g * v) for g, x in enumerate(digits)) == d
                for qj in primes:
                    sim.sim_bfvsel_diff_digits(odd, even, qi, E, v, qj, buf)
                    assert list(buf[:E]) == [x % qj for x in digits], (qi, qj, v, odd, even)


def test_tail_add(sim, primes):
    rng = np.random.default_rng(32)
    for q in primes:
        for prod, even in operands(q, rng):
            assert sim.sim_bfvsel_add(prod, even, q) == (prod + even) % q, (q, prod, even)


def test_symbol_exported_declared_and_bound(be):
    s = "he355_bfv_select"
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    assert hasattr(lib, s)
    assert s in be.C_ABI_SYMBOLS and (s + "(") in hdr
    assert hasattr(be.Context, "bfv_select")
