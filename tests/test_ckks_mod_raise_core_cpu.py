"""The arithmetic of the CKKS modulus raise on the CPU (tests/csim/sim_raise.cpp runs csrc/raise_core.h -- the functions the HIP kernels
k_raise_lift and k_raise_cols compile) against Python integers, in both builds of the u64 engine.  For each (q_0, q_j) pair of every chain the
device test uses -- {60, 40, 40, 60}, {40, 60, 60}, {60, 60, 60}, {42, 38, 45, 44}, {60, 50, 40, 60} at N = 2048, and from
tests/explicit_moduli.py `tiny` (a 60-bit prime 0 over 14-bit moduli), `engine_edge_47` and the primes of `ratio_two` with the 47- and the 46-bit
one as prime 0 (q_0 on either side of 2 q_j) -- the operands

* 0, 1, q_0 - 1, both tie points (q_0 - 1) / 2 and (q_0 + 1) / 2;
* |c| = q_j, 2 q_j, the largest multiple of q_j below q_0 / 2 and their neighbours, on both signs: the `r == 0` branch of the negation and
  both sides of the `v >= q_j` edge of the reduction;
* uniform values

give c mod q_j, canonical: in the integer form under every target, and under every fp64-engine target (q_j < 2^47) in the form k_raise_cols
picks from q_0 (narrow below 2^52: the double itself, re-centred where q_0 > 2 q_j; wide: hi * (2^32 mod q_j) + lo), whose lazy value stays
within q_j (the column pass's input range).  The host rule of the small-batch split is restated.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ckks_mod_raise_ref as ref
import csim_lib
import explicit_moduli as em

u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
N = 2048
BITS = {"60_40_40_60": [60, 40, 40, 60], "40_60_60": [40, 60, 60], "60_60_60": [60, 60, 60], "42_38_45_44": [42, 38, 45, 44], "60_50_40_60": [60, 50, 40, 60]}
RATIO = em.load()["ratio_two"]["primes"]  # [45-bit q_t, 46-bit just below 2 q_t, 47-bit just above, 60-bit special]
EXPLICIT = {
    "tiny": em.load()["tiny"]["primes"],
    "engine_edge_47": em.load()["engine_edge_47"]["primes"],
    "ratio_two_above": [RATIO[2], RATIO[0], RATIO[1], RATIO[3]],  # q_0 > 2 q_1: re-centred
    "ratio_two_below": [RATIO[1], RATIO[0], RATIO[2], RATIO[3]],  # q_0 < 2 q_1: as it is
}


def declare(L):
    L.sim_raise_lift_u64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]
    L.sim_raise_lift_u64.restype = None
    L.sim_raise_lift_f64.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, f64p]
    L.sim_raise_lift_f64.restype = C.c_int
    L.sim_raise_tsplit.argtypes = [C.c_uint64, C.c_int, C.c_uint64]
    L.sim_raise_tsplit.restype = C.c_int
    return L


@pytest.fixture(scope="module", params=[False, True], ids=["shoup", "fold"])
def sim(request):
    return declare(csim_lib.load(fold=request.param))


def chain_moduli(oracle, name):
    if name in EXPLICIT:
        return [int(q) for q in EXPLICIT[name][:-1]]
    o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=BITS[name], sec128=False)
    return [int(q) for q in o.moduli[:-1]]


@pytest.mark.parametrize("chain", list(BITS) + list(EXPLICIT))
def test_the_centred_lift_at_its_edges(sim, oracle, chain):
    q = chain_moduli(oracle, chain)
    q0 = q[0]
    rng = np.random.default_rng(len(chain))
    for qj in q:  # (q_j = q_0 too: the lift returns the input)
        ops = ref.edge_operands(q0, qj) + [int(v) for v in rng.integers(0, q0, 257, dtype=np.uint64)]
        x = np.array(ops, dtype=np.uint64)
        want = [int(c) % qj for c in ref.centred(x, q0)]
        out = np.empty(len(x), dtype=np.uint64)
        sim.sim_raise_lift_u64(len(x), q0, qj, x.ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        assert [int(v) for v in out] == want, (chain, hex(qj), "integer form")
        if qj == q0:
            assert np.array_equal(out, x)
        if em.is_f64(qj):
            lazy = np.empty(len(x), dtype=np.float64)
            wide = sim.sim_raise_lift_f64(len(x), q0, qj, x.ctypes.data_as(u64p), out.ctypes.data_as(u64p), lazy.ctypes.data_as(f64p))
            assert wide == (1 if q0 >> 52 else 0)
            assert [int(v) for v in out] == want, (chain, hex(qj), "fp64 form")
            assert float(lazy.max()) <= qj, (chain, hex(qj), "the lazy value leaves the column pass's range")


def test_both_sides_of_two_q_are_met():
    above, below = EXPLICIT["ratio_two_above"], EXPLICIT["ratio_two_below"]
    assert above[0] > 2 * above[1] and below[0] < 2 * below[1] and above[0] - 2 * above[1] < above[0] >> 20 and 2 * below[1] - below[0] < below[0] >> 20
    tiny = EXPLICIT["tiny"]
    assert tiny[0].bit_length() == 60 and tiny[1].bit_length() == 14


def test_the_split_rule(sim):
    for cus in (1, 64, 256, 304):
        for polys in (1, 2, 3, 6, 16, 63, 64, 65, 76, 77, 1000):
            for L_to in (1, 2, 3, 4, 16, 30):
                assert sim.sim_raise_tsplit(polys, L_to, cus) == ref.tsplit_rule(polys, L_to, cus), (cus, polys, L_to)
    assert ref.tsplit_rule(1, 16, 256) == 15 and ref.tsplit_rule(2, 6, 256) == 5 and ref.tsplit_rule(64, 6, 256) == 1 and ref.tsplit_rule(63, 6, 256) == 2
