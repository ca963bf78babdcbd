"""The rescale tail of the fused ct x ct multiply -> relinearize -> rescale, as exact integers (no GPU, no oracle).

key_switch_tail brings the divided-out prime q_last = q_{L-1} to coefficient form in one of two orders:

  present order   (every source but the operand-formed product)  the special-prime correction delta1 goes through the forward
                  transform, the floor step runs in NTT form, md = (sums - NTT(delta1)) * P^-1 + addend, and md comes back through
                  the inverse transform;
  short order     (operand-formed sums: key residues scaled by P^-1, addend inside the sums)  sums' = sums * P^-1 + addend go
                  through the inverse transform as they are and c' = iNTT(sums') - P^-1 * delta1 mod q_last is formed in
                  coefficient form (k_floor_colsn, sub2).

Both must give the same canonical residue, hence the same combined correction delta2 + P^-1 * delta1 for every other prime and the same
rescaled result -- and all of it must be what the definitions say (tests/golden/exact_model.py: CRT composition and exact floors).
Parameters are the fixtures' prime chains (exact_vectors.json: toy rings; exact_vectors_big.json: the bench ring N = 2^15, L = 16),
inputs are exact_inputs' seeded uniform residues."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import exact_inputs as xi  # noqa: E402
from exact_model import Ring  # noqa: E402

FIX = json.load(open(os.path.join(HERE, "golden", "exact_vectors.json")))
BIG = json.load(open(os.path.join(HERE, "golden", "exact_vectors_big.json")))
CASES = [(n, f) for n, f in FIX.items() if f["scheme"] == "ckks"] + [(n, f) for n, f in BIG.items() if f["scheme"] == "ckks" and "multiply_relin_rescale" in f["expected"]]


def inv(a, q):
    return pow(a % q, q - 2, q)


@pytest.mark.parametrize("name,f", CASES, ids=[n for n, _ in CASES])
def test_short_order_equals_present_order_and_the_exact_floors(name, f):
    primes = [int(p, 16) for p in f["primes"]]
    N, seed, K = f["N"], f["seed"], len(primes)
    L, sp = K - 1, K - 1
    last = L - 1
    assert L >= 2
    R = Ring(N, primes)
    P, ql = primes[sp], primes[last]
    hP, hl = P // 2, ql // 2
    # coefficient form of the key-product sums under the data primes and the special prime, and of the addend (c0 or c1)
    T = {t: xi.uniform_poly(seed, 700 + t, primes[t], N) for t in list(range(L)) + [sp]}
    C = [xi.uniform_poly(seed, 800 + i, primes[i], N) for i in range(L)]
    r1 = [(s + hP) % P for s in T[sp]]  # special-prime sums + floor(P/2), canonical (k_floor_colsn's source column)

    def delta1(i):
        q = primes[i]
        return [(r % q - hP % q) % q for r in r1]

    # ---- the divided-out prime, through the transforms --------------------------------------------------------------------------
    Pinv = inv(P, ql)
    sums_ntt, add_ntt = R.ntt(last, T[last]), R.ntt(last, C[last])
    d1 = delta1(last)
    d1_ntt = R.ntt(last, d1)
    md_ntt = [((s - d) * Pinv + a) % ql for s, d, a in zip(sums_ntt, d1_ntt, add_ntt)]
    c_present = R.intt(last, md_ntt)
    sums_s_ntt = [(s * Pinv + a) % ql for s, a in zip(sums_ntt, add_ntt)]  # what relin_scaled keys and tensor_init accumulate
    x = R.intt(last, sums_s_ntt)
    c_short = [(v - Pinv * d) % ql for v, d in zip(x, d1)]
    assert all(0 <= v < ql for v in c_short)
    assert c_short == c_present
    # ---- ... and both are the definition: floor((S + floor(P/2)) / P) + addend, S the representative in [0, Q P) -------------------
    idx = list(range(L)) + [sp]
    _, compose_qp = R.crt(idx)
    down = [(compose_qp([T[t][n] for t in idx]) + hP) // P for n in range(N)]
    assert c_short == [(v + a) % ql for v, a in zip(down, C[last])]
    # ---- every other prime: the combined correction and the rescaled residue -------------------------------------------------------
    md = [[(v + a) % primes[i] for v, a in zip(down, C[i])] for i in range(L)]  # the mod-down result, by definition
    _, compose_q = R.crt(list(range(L)))
    resc = [(compose_q([md[i][n] for i in range(L)]) + hl) // ql for n in range(N)]  # the rescale, by definition
    for j in range(last):
        q = primes[j]
        Pj, qlj = inv(P, q), inv(ql, q)
        d1j = delta1(j)

        def combined(c):  # delta2 + P^-1 * delta1 from the divided-out prime's coefficients c
            return [(((v + hl) % ql) % q - hl % q + Pj * d) % q for v, d in zip(c, d1j)]

        comb_present, comb_short = combined(c_present), combined(c_short)
        assert comb_short == comb_present
        # present order, two floor steps one after the other
        md_j = [((s - d) * Pj + a) % q for s, d, a in zip(T[j], d1j, C[j])]
        assert md_j == md[j]
        two_step = [((m - (((v + hl) % ql) % q - hl % q)) * qlj) % q for m, v in zip(md_j, c_present)]
        # fused epilogue on scaled sums (floor_fin2_s): (sums' - combined) * q_last^-1
        fused = [(((s * Pj + a) - d) * qlj) % q for s, a, d in zip(T[j], C[j], comb_short)]
        assert fused == two_step
        assert fused == [v % q for v in resc]
