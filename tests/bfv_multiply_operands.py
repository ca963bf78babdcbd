"""The operand families of the BEHZ multiply tests (test_gpu_parity_bfv.py, test_gpu_bfv_multiply_routes.py, test_oracle_bfv_multiply_model_cpu.py):
polynomials that drive every bound of the Shenoy-Kumaresan step to its extreme, built for a level's own Q = q_0 .. q_(L-1).  All
coefficients +-floor(Q/2) with the signs that make the negacyclic sums of coefficient N - 1 (no wrapped terms) and of coefficient 0 (all but
one term wrapped) as large as they get, and all coefficients Q - 1 / 0 / 1."""
import numpy as np

# the ciphertexts (polynomial 0, polynomial 1) the families are paired into
FAMILY_CTS = [("plus_half", "plus_half"), ("minus_half", "plus_half"), ("alternating", "alternating"), ("first_negative", "minus_half"),
              ("q_minus_1", "q_minus_1"), ("zero", "one"), ("q_minus_1", "plus_half")]


def residues(o, values, L):
    """Integer coefficient vector(s) -> residues [.., L, N] under the first L moduli."""
    return np.stack([np.array([int(v) % q for v in values], dtype=np.uint64) for q in o.moduli[:L]])


def family_polys(o, L, N):
    """{family: [L][N]} at level L"""
    Q = 1
    for q in o.moduli[:L]:
        Q *= int(q)
    h = Q // 2
    mods = [int(q) for q in o.moduli[:L]]

    def const(v):
        return np.stack([np.full(N, v % q, dtype=np.uint64) for q in mods])

    alt = const(h)                   # +Q/2, -Q/2 alternating
    alt[:, 1::2] = const(h + 1)[:, 1::2]
    first_neg = const(h)             # coefficient 0: -a_0 b_0 ... all wrapped terms add up
    first_neg[:, 0] = const(h + 1)[:, 0]
    return {"plus_half": const(h), "minus_half": const(h + 1), "alternating": alt, "first_negative": first_neg, "q_minus_1": const(Q - 1),
            "zero": const(0), "one": const(1)}


def family_cts(o, L, N):
    """the seven family ciphertexts [2][L][N] of FAMILY_CTS, in that order"""
    polys = family_polys(o, L, N)
    return [np.stack([polys[x], polys[y]]) for x, y in FAMILY_CTS]
