"""Chains of explicit moduli (a plain helper module: tests/golden/make_explicit_moduli.py, tests/test_explicit_moduli_cpu.py,
tests/test_gpu_explicit_moduli.py and tests/test_gpu_bfv_chain_layouts.py import it).

Every other context of the suite takes its moduli from the prime-size rule (the largest primes 1 (mod 2N) below 2^bits, the largest
batching plain modulus), so every prime the kernels meet is 2^b - (small).  The library admits any NTT-friendly prime below 2^60 and any
plain modulus 2 <= t < 2^32, and several device-side decisions are functions of the prime itself.  This module restates those decisions
in Python -- it does not link them; tests/test_explicit_moduli_cpu.py holds each restatement to the library's host side -- and loads
tests/golden/explicit_moduli.json, the pinned chains that sit on both sides of each of them.

    engine        q < 2^47: the fp64 engine, else the u64 engine                                   (he_params.cpp, Params::build)
    fold form     every chain prime >= 2^47 is 2^60 - c with 0 < c < 2^26, else the Shoup form     (modarith.h, fold_prime_ok)
    lift class    of (digit prime q_j, fp64 target q_t) in k_k2n: direct, lift or general          (device_tables.h, k2_lift_class)
    direct floor  acc_terms of an fp64 prime: 0 above the x-bound, else floor(2^49 / term bound)   (modarith.h, floor_direct_terms)
    mac run       floor((2^128 - 1) / (q - 1)^2), capped at 2^16                                   (bfv_mac_core.h, bfv_mac_run)

The floating-point restatements use the same operations in the same order as the C++ (doubles, one rounding per operation), so they
agree to the bit."""
from __future__ import annotations

import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "explicit_moduli.json")
EPS51 = 4.440892098500626e-16  # 2^-51, as the C++ writes it
TWO47, TWO49 = 140737488355328.0, 562949953421312.0
FOLD_MAX_C = 1 << 26
TENSOR_TERMS = 3  # modarith.h: kTensorTerms
AUX_BITS = 46     # he_params.h: kAuxBits


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def is_f64(q: int) -> bool:
    return q >> 47 == 0


def fold_c(q: int) -> int:
    return (1 << 60) - q


def fold_prime_ok(q: int) -> bool:
    return q >> 59 == 1 and q >> 60 == 0 and fold_c(q) < FOLD_MAX_C


def form_of(moduli):
    """the form of the u64 engine over the whole chain, the key prime included; None where no prime belongs to it"""
    wide = [q for q in moduli if not is_f64(q)]
    if not wide:
        return None
    return "fold" if all(fold_prime_ok(q) for q in wide) else "shoup"


def stage_growth(m: float, q: float, stages: int) -> float:
    """a stage of the fp64 butterfly takes |.| <= m to m + q (1/2 + m 2^-51)"""
    for _ in range(stages):
        m += q * (0.5 + m * EPS51)
    return m


def lift_class(qj: int, qt: int, logn1: int) -> str:
    """k_k2n's class of digit prime q_j under fp64-engine target q_t: "direct" (the digit enters the column pass as it is), "lift" (it is
    re-centred first, or arrives reduced from a prime of 52 bits and more), both with 48-bit packed rows, or "general" """
    assert is_f64(qt)
    df = qj >> 52 == 0
    direct = df and not qj > 2 * qt
    m = (float(qj) if direct else 0.5 * float(qt) + 1.0) if df else float(qt)
    m = stage_growth(m, float(qt), logn1)
    if not m * 1.0000001 < TWO47:
        return "general"
    return "direct" if direct else "lift"


def fits48_wide(qt: int, logn1: int) -> bool:
    """does a digit of a prime of 52 bits and more (entry magnitude q_t) keep the 48-bit rows under target q_t?  Monotone in q_t"""
    return lift_class((1 << 60) - 1, qt, logn1) != "general"


def x_bound(q: int) -> float:
    return stage_growth(4.0 * float(q), float(q), 15)


def term_bound(q: int) -> float:
    qd = float(q)
    return qd * (0.5 + stage_growth(TWO47, qd, 10) * EPS51)


def direct_terms(q: int) -> int:
    if not is_f64(q):
        return 0
    if not x_bound(q) <= TWO49:
        return 0
    t = TWO49 / term_bound(q)
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def mac_run(q: int) -> int:
    if q < 3:
        return 1 << 16
    return min(1 << 16, ((1 << 128) - 1) // ((q - 1) ** 2))


def bisect_last_true(pred, lo: int, hi: int) -> int:
    """the largest v in [lo, hi) with pred(v), pred monotone (true, then false); pred(lo) must hold and pred(hi) must not"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
def load() -> dict:
    """{id: {"N", "primes" (ints, special prime last), "t" (0: CKKS), "for", ...}}"""
    with open(FIXTURE) as f:
        doc = json.load(f)
    out = {}
    for e in doc["chains"]:
        c = dict(e)
        c["primes"] = [int(p, 16) for p in e["primes"]]
        out[e["id"]] = c
    return out


def all_primes(chains: dict) -> list:
    """[(N, q)], every distinct pair of the fixture"""
    return sorted({(c["N"], q) for c in chains.values() for q in c["primes"]})


def bits_of(primes) -> list:
    return [int(q).bit_length() for q in primes]
