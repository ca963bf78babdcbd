"""The operands of the complex CKKS codec tests and of their fixture tests/golden/ckks_complex_vectors.json (exact values by mpmath:
tests/golden/make_ckks_complex_vectors.py), and the bounds against it: the real codec's (tests/client_operands.py), part by part.  TEST-ONLY."""
import ctypes as C
import json
import os

import numpy as np

import client_operands as co

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckks_complex_vectors.json")
SCALE = 2.0 ** 40
DECODE_LEVELS = {"c60x4": [4], "c45x15": [1, 8, 16]}  # the decode cases of client_edge_vectors.json whose imaginary parts the fixture holds


def counts(N):
    return (1, N // 2 - 1, N // 2)


def complex_input(N, count):
    """`count` complex slots, both parts uniform in [-0.7, 0.7] (inside the unit disc); the generator's bits alone, no library function"""
    rng = np.random.default_rng(7000 + N + count)
    return (rng.uniform(-0.7, 0.7, count) + 1j * rng.uniform(-0.7, 0.7, count)).astype(np.complex128)


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def check_encode_case(fixture, case, coeffs, who):
    """the real encoder's bound (co.check_encode_case): within ENCODE_FACTOR * E_np of the exact coefficients at the sampled positions"""
    pos = fixture["positions"][str(case["N"])]
    err = max(abs(coeffs[p] * 65536 - int(x)) for p, x in zip(pos, case["exact_x65536"])) / 65536.0
    bound = co.ENCODE_FACTOR * float.fromhex(case["E_np"])
    assert err <= bound, (who, case["id"], err, bound)
    return err


def check_decode_case(case, slot_positions, im, who):
    """the real decoder's slot bound (co.check_decode_case) on the imaginary parts: within DECODE_FACTOR * E_np_im of the exact ones"""
    exact = np.array([float.fromhex(x) for x in case["exact_im"]])
    got = np.asarray(im, dtype=np.float64)[slot_positions]
    assert np.all(np.isfinite(got)), (who, case["id"])
    err = float(np.max(np.abs(got - exact)))
    bound = co.DECODE_FACTOR * float.fromhex(case["E_np_im"])
    assert err <= bound, (who, case["id"], err, bound)
    return err


class ComplexHost(co.HostClient):
    """the product's host client with the complex codec (tests/csim/sim_cplx.cpp), numpy complex128 in and out"""

    def __init__(self, S, N, bits):
        S.simc_ckks_encode_complex.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_double, C.POINTER(C.c_uint64)]
        S.simc_ckks_encode_complex.restype = None
        S.simc_ckks_decode_complex.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_double, C.POINTER(C.c_double)]
        S.simc_ckks_decode_complex.restype = None
        super().__init__(S, "ckks", N, bits)

    def ckks_encode_complex(self, values, scale):
        v = np.ascontiguousarray(values, dtype=np.complex128)
        out = np.empty((self.Ltop, self.N), dtype=np.uint64)
        self.S.simc_ckks_encode_complex(self.c, v.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)), len(v), scale, self._u(out))
        return out

    def ckks_decode_complex(self, plain_ntt, scale):
        out = np.empty(self.N // 2, dtype=np.complex128)
        self.S.simc_ckks_decode_complex(self.c, self._u(np.ascontiguousarray(plain_ntt)), plain_ntt.shape[0], scale, out.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        return out
