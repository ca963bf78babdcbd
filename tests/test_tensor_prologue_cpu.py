"""The ct x ct prologue of k_k3<TENSOR> from three products (csrc/modarith.h: dy_mul3 -- c0 = a0 b0, c2 = a1 b1,
c1 = (a0 + a1)(b0 + b1) - c0 - c2) held to Python integers, on both engines, and the host-side rule that lets the fp64 engine's floor
steps read the sums as they are, with the term count such a launch now passes (L + kTensorTerms).

tests/tensor_prologue_host.cpp includes the header and is compiled here with the host compiler, once per form of the u64 engine
(HE355_U64_FOLD = 0 / 1), and loaded through ctypes.

Bounds asserted (none taken from what the code returns):
  * one centred product is at most floor_term_bound(q) = q (1/2 + X 2^-51), X the widest digit; restated below in exact rationals;
  * c0, c2 are one term each, c1 is kTensorTerms = 3 of them, the c1 sum after t key products 3 + t;
  * where the rule admits the direct forms for L + 3 terms, (L + 3) terms and the correction row stay inside 2^49."""
import ctypes as C
import itertools
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reference-seal-backend_amd", "csrc")
N_RANDOM = 4000
B49 = 1 << 49

with open(os.path.join(HERE, "golden", "primes.json")) as _f:
    _G = json.load(_f)
ALL_PRIMES = sorted({int(p, 16) for e in _G["get_primes"] + _G["chains"] for p in e["primes"]})
HEADLINE = next([int(p, 16) for p in c["primes"]] for c in _G["chains"] if c["N"] == 32768 and c["bit_sizes"] == [60] + [45] * 15 + [60])


def _prime(bits):
    """the largest golden prime of that bit size; 47 bits has none in the golden chains: the largest prime 1 (mod 2^16) below 2^47"""
    got = [p for p in ALL_PRIMES if p.bit_length() == bits]
    if got:
        return got[-1]
    q = (1 << bits) - (1 << 16) + 1
    while not all(pow(a, q - 1, q) == 1 for a in (2, 3, 5, 7, 11, 13)) or any(q % d == 0 for d in range(3, 2000, 2)):
        q -= 1 << 16
    return q


Q45, Q47, Q60 = _prime(45), _prime(47), _prime(60)
u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)


@pytest.fixture(scope="module", params=[0, 1], ids=["shoup_build", "fold_build"])
def lib(request, tmp_path_factory):
    fold = request.param
    so = str(tmp_path_factory.mktemp("tensor_prologue") / f"libtensor_prologue_{fold}.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-DHE355_U64_FOLD={fold}", "-I", CSRC,
                    os.path.join(HERE, "tensor_prologue_host.cpp"), "-o", so], check=True)
    S = C.CDLL(so)
    assert S.tp_fold_build() == fold
    S.tp_tensor_terms.restype = S.tp_direct_terms.restype = C.c_uint32
    S.tp_direct_terms.argtypes = [C.c_uint64]
    S.tp_direct.argtypes = [C.c_uint32, C.c_uint32]
    S.tp_term_bound.restype = S.tp_acc_max.restype = C.c_double
    S.tp_term_bound.argtypes = [C.c_uint64]
    S.tp_f64.restype = S.tp_u64.restype = None
    S.tp_f64.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, u64p, u64p, u64p, u64p, C.c_int, f64p, u64p, f64p, f64p, f64p, f64p, f64p, u64p]
    S.tp_u64.argtypes = [C.c_uint64, C.c_size_t, u64p, u64p, u64p, u64p, C.c_int, u64p, u64p, u64p, u64p, u64p, u64p, C.POINTER(C.c_int)]
    return S


def operands(q):
    """a0, a1, b0, b1: every combination of {0, 1, q - 1, floor(q/2), floor(q/2) + 1} (625), then N_RANDOM seeded uniform residues"""
    edge = [0, 1, q - 1, q // 2, q // 2 + 1]
    grid = np.array(list(itertools.product(edge, repeat=4)), dtype=np.uint64)
    rng = np.random.default_rng(q % (1 << 32) + 5)
    rnd = rng.integers(0, q, (N_RANDOM, 4), dtype=np.uint64)
    allv = np.concatenate([grid, rnd])
    return [np.ascontiguousarray(allv[:, k]) for k in range(4)]


def want_tensor(q, a0, a1, b0, b1):
    A0, A1, B0, B1 = ([int(v) for v in x] for x in (a0, a1, b0, b1))
    c0 = [(x * y) % q for x, y in zip(A0, B0)]
    c1 = [(x * w + z * y) % q for x, z, y, w in zip(A0, A1, B0, B1)]
    c2 = [(z * w) % q for z, w in zip(A1, B1)]
    return c0, c1, c2


def stage_growth(m, q, stages):
    """the fp64 butterfly's growth rule in exact rationals (modarith.h: f64_stage_growth)"""
    m = Fraction(m)
    for _ in range(stages):
        m += q * (Fraction(1, 2) + m / (1 << 51))
    return m


def term_bound(q):
    """one centred product x * key, key canonical, x the widest digit: 2^47 out of the packed row, then 10 row stages"""
    return q * (Fraction(1, 2) + stage_growth(1 << 47, q, 10) / (1 << 51))


def maximal_terms(q, terms, xmax, sign=1):
    """`terms` pairs (x, key), |x| = xmax (an integer), key canonical, whose centred product is as close to sign * q/2 as a residue gets:
    every term pushes the sum the same way"""
    x = int(xmax)
    while x % q == 0:
        x -= 1
    target = (q // 2) if sign > 0 else (q - q // 2)
    key = (target * pow(x % q, -1, q)) % q
    return [x] * terms, [key] * terms


@pytest.mark.parametrize("q", [Q45, Q47], ids=["45bit", "47bit"])
def test_f64_three_products_and_the_sums_they_start(lib, q):
    assert q.bit_length() in (45, 47) and lib.tp_tensor_terms() == 3
    a0, a1, b0, b1 = operands(q)
    n = len(a0)
    w0, w1, w2 = want_tensor(q, a0, a1, b0, b1)
    per = lib.tp_term_bound(q)
    assert per == pytest.approx(float(term_bound(q)), rel=1e-12)
    s2 = Q45 if q != Q45 else HEADLINE[1]
    inv2 = pow(s2 % q, -1, q)
    L = 16
    xmax = int(stage_growth(1 << 47, q, 10))  # the widest digit the key product is handed
    for sign in (1, -1):
        xs, keys = maximal_terms(q, L, xmax, sign)
        x = np.array(xs, dtype=np.float64)
        key = np.array(keys, dtype=np.uint64)
        assert int(x[0]) == xs[0]
        rng = np.random.default_rng(q % (1 << 32) + 11)
        corr = rng.integers(-(q // 2), q // 2, n, endpoint=True).astype(np.float64)
        c0, c1, c2, s1 = (np.empty(n, dtype=np.float64) for _ in range(4))
        fin2 = np.empty(n, dtype=np.uint64)
        lib.tp_f64(q, s2, n, a0.ctypes.data_as(u64p), a1.ctypes.data_as(u64p), b0.ctypes.data_as(u64p), b1.ctypes.data_as(u64p), L,
                   x.ctypes.data_as(f64p), key.ctypes.data_as(u64p), corr.ctypes.data_as(f64p), c0.ctypes.data_as(f64p), c1.ctypes.data_as(f64p),
                   c2.ctypes.data_as(f64p), s1.ctypes.data_as(f64p), fin2.ctypes.data_as(u64p))
        for got in (c0, c1, c2, s1):
            assert (np.rint(got) == got).all() and float(np.abs(got).max()) < 2.0 ** 52  # exact integers in the doubles
        # magnitudes: one term each for c0 and c2, kTensorTerms for c1, L more behind the digit loop
        assert float(np.abs(c0).max()) <= per and float(np.abs(c2).max()) <= per and float(np.abs(c2).max()) < q
        assert float(np.abs(c1).max()) <= 3 * per
        assert float(np.abs(s1).max()) <= (L + 3) * per
        assert float(np.abs(s1).max()) >= (L - 1) * (q // 2)  # the terms were maximal: the sum went where the bound lets it
        # residues
        tail = sum(xx * kk for xx, kk in zip(xs, keys))
        for name, got, want in (("c0", c0, w0), ("c1", c1, w1), ("c2", c2, w2), ("sum", s1, [(w + tail) % q for w in w1])):
            g = [int(v) % q for v in got]
            bad = [i for i in range(n) if g[i] != want[i]]
            assert not bad, (name, hex(q), len(bad), bad[0], int(a0[bad[0]]), int(a1[bad[0]]), int(b0[bad[0]]), int(b1[bad[0]]))
        # the floor step that reads the sum as it is: exact wherever the host-side rule admits it for this launch
        if lib.tp_direct(lib.tp_direct_terms(q), L + 3):
            assert float(np.abs(s1).max()) <= B49 == lib.tp_acc_max()
            want = [((int(s) - int(c)) * inv2) % q for s, c in zip(s1, corr)]
            assert [int(v) for v in fin2] == want
    if q == Q45:
        assert lib.tp_direct(lib.tp_direct_terms(q), L + 3) == 1
    else:
        assert lib.tp_direct_terms(q) == 0  # a 47-bit prime re-centres first (floor_prep), whatever the term count


@pytest.mark.parametrize("q", [Q45, Q47, Q60], ids=["45bit", "47bit", "60bit"])
def test_u64_three_products_and_the_sums_they_start(lib, q):
    fold = lib.tp_fold_build()
    if fold and q != Q60:
        assert (1 << 60) - q >= 1 << 26  # the fold build of the u64 engine runs primes 2^60 - c only: nothing to hold here
        return
    a0, a1, b0, b1 = operands(q)
    n = len(a0)
    w0, w1, w2 = want_tensor(q, a0, a1, b0, b1)
    L = 16
    top = 8 * q if fold else 12 * q  # what the wide lazy row pass hands the key product (ArU64::bfly_fwd_lazy)
    rng = np.random.default_rng(q % (1 << 32) + 13)
    for xs, keys in (([top - 1] * L, [q - 1] * L), ([int(v) for v in rng.integers(0, top, L, dtype=np.uint64)], [int(v) for v in rng.integers(0, q, L, dtype=np.uint64)])):
        x, key = np.array(xs, dtype=np.uint64), np.array(keys, dtype=np.uint64)
        c0, c1, c2, s1 = (np.empty(n, dtype=np.uint64) for _ in range(4))
        ovf = C.c_int(0)
        lib.tp_u64(q, n, a0.ctypes.data_as(u64p), a1.ctypes.data_as(u64p), b0.ctypes.data_as(u64p), b1.ctypes.data_as(u64p), L,
                   x.ctypes.data_as(u64p), key.ctypes.data_as(u64p), c0.ctypes.data_as(u64p), c1.ctypes.data_as(u64p), c2.ctypes.data_as(u64p),
                   s1.ctypes.data_as(u64p), C.byref(ovf))
        assert ovf.value == 0
        tail = sum(xx * kk for xx, kk in zip(xs, keys))
        for name, got, want in (("c0", c0, w0), ("c1", c1, w1), ("c2", c2, w2), ("sum", s1, [(w + tail) % q for w in w1])):
            assert int(got.max()) < q, name  # canonical, as the accumulators and the own digit's key product take them
            g = [int(v) for v in got]
            bad = [i for i in range(n) if g[i] != want[i]]
            assert not bad, (name, hex(q), len(bad), bad[0], int(a0[bad[0]]), int(a1[bad[0]]), int(b0[bad[0]]), int(b1[bad[0]]))


def test_term_rule_admits_the_direct_forms_only_where_the_worst_case_fits(lib):
    """every chain of tests/golden/primes.json (what the tests build contexts from), every level 1 <= L <= K - 1, every fp64-engine prime as
    the target: L + kTensorTerms terms pass floor_direct only where that many worst-case terms and the correction row, in exact rationals,
    stay inside 2^49"""
    kt = lib.tp_tensor_terms()
    seen = 0
    for c in _G["chains"]:
        primes = [int(p, 16) for p in c["primes"]]
        K = len(primes)
        for q in (p for p in primes if p < 1 << 47):
            T = lib.tp_direct_terms(q)
            per, xb = term_bound(q), stage_growth(4 * q, q, 15)
            # the third operand product multiplies two values below 2q: the bound of |x| = 4q against a canonical key, inside one term's
            assert q * (Fraction(1, 2) + Fraction(4 * q, 1 << 51)) <= per
            for L in range(1, max(2, K)):
                if lib.tp_direct(T, L + kt):
                    assert (L + kt) * per <= B49 and xb <= B49, (c["N"], c["bit_sizes"], hex(q), L)
                    seen += 1
    assert seen
    # the headline's chain keeps the direct forms at L = 16 (and below), with three operand terms
    for q in HEADLINE[1:-1]:
        assert q.bit_length() == 45
        for L in range(1, 17):
            assert lib.tp_direct(lib.tp_direct_terms(q), L + kt) == 1, (hex(q), L)
    # a 45-bit prime: 24 terms, so L <= 21 now; 46- and 47-bit primes never
    t45 = lib.tp_direct_terms(HEADLINE[1])
    assert lib.tp_direct(t45, 21 + kt) == 1 and lib.tp_direct(t45, 22 + kt) == 0
    assert lib.tp_direct_terms(Q47) == 0
