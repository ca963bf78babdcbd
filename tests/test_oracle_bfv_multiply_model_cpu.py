"""`oracle.bfv_multiply` -- the reference every BEHZ multiply on the device is held to -- against the exact integer model
(tests/golden/exact_model.py, Model.bfv_multiply: big integers, no auxiliary primes, no NTT) where test_exact_model.py does not pin it: at
levels below a chain's top level, at four data primes ({60, 40, 40, 40}, and {60 x 4} with a 31-bit plain modulus: the most auxiliary
primes per data prime), and on the operand families of bfv_multiply_operands.py built for the level's own Q (all coefficients
+-floor(Q/2) in the sign patterns that drive the Shenoy-Kumaresan bounds to their ends, Q - 1, 0 and 1) as well as a uniform pair.  N = 1024:
the model is computed live.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from exact_model import Model  # noqa: E402

from bfv_multiply_operands import FAMILY_CTS, family_cts  # noqa: E402

N = 1024
CASES = [
    # bit sizes (special prime last), plain bits, level
    ("d4_top", [60, 40, 40, 40, 60], 20, 4),
    ("d4_below_top", [60, 40, 40, 40, 60], 20, 2),
    ("d4_one_prime", [60, 40, 40, 40, 60], 20, 1),
    ("60x4_top", [60, 60, 60, 60, 60], 31, 4),
    ("60x4_below_top", [60, 60, 60, 60, 60], 31, 3),
    ("shoup_below_top", [50, 40, 50], 20, 1),
]
# (operand a, operand b): indices into the seven family ciphertexts + [uniform, uniform]
PAIRS = [(0, 0), (1, 2), (3, 1), (2, 3), (4, 4), (4, 6), (5, 4), (7, 8), (7, 2)]


@pytest.mark.parametrize("name,bits,pb,L", CASES, ids=[c[0] for c in CASES])
def test_oracle_bfv_multiply_equals_the_integer_model(oracle, name, bits, pb, L):
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    assert 1 <= L <= o.L and (("below" not in name and "one_prime" not in name) == (L == o.L))
    assert len(FAMILY_CTS) == 7 and int(o.t).bit_length() == pb
    M = Model(N, [int(q) for q in o.moduli], ntt_form=False)
    rng = np.random.default_rng(900 + L)
    cts = family_cts(o, L, N) + [o.random_poly(rng, L, 2) for _ in range(2)]
    for ia, ib in PAIRS:
        a, b = cts[ia], cts[ib]
        want = np.array(M.bfv_multiply(a.tolist(), b.tolist(), int(o.t)), dtype=np.uint64)
        got = o.bfv_multiply(a, b)
        assert got.shape == want.shape == (3, L, N)
        assert np.array_equal(got, want), (name, ia, ib, np.argwhere(got != want)[:1].tolist())
