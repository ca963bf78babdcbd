"""What the BFV GPU test modules share (test_gpu_bfv_levels.py, test_gpu_bfv_noise.py, test_gpu_bfv_ntt_form.py): the parameter chains, the
`be` fixture (imported by name), the device / oracle context pair, random operands and the check of a refused call."""
import importlib

import numpy as np
import pytest

CONFIGS = {
    # the CONFIGS of tests/test_gpu_parity_bfv.py
    "n1024": (1024, [50, 40, 50], 20),            # the Shoup form of the u64 engine (50-bit primes are not 2^60 - c)
    "n4096_d3": (4096, [60, 40, 40, 60], 20),     # the fold form
    "n8192_default": (8192, [60, 40, 60], 20),
    "n32768_d3": (32768, [60, 40, 40, 60], 20),
}


def random_chain(seed):
    """the draw of test_gpu_parity_bfv.py::test_bfv_random_parameter_chains"""
    rng = np.random.default_rng(5000 + seed)
    N = int(rng.choice([1024, 2048, 4096]))
    K = int(rng.integers(2, 6))
    bits = [int(b) for b in rng.integers(35, 61, K)]
    return N, bits, int(rng.integers(16, 23))


ALL = dict(CONFIGS)
for _s in (0, 3, 4):
    ALL[f"random{_s}"] = random_chain(_s)

SENT = np.uint64(0x5E17155E17155E17)


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device")
    return mod


def pair(be, oracle, chain, keys=False):
    """(g, o, N, sk, pk): a device context and the oracle's of one chain -- a name of ALL, or (N, bit sizes, plain bits) itself; keys: the
    oracle's secret and public key, set on the device (else None)"""
    N, bits, pb = ALL[chain] if isinstance(chain, str) else chain
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False, device=0)
    o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=bits, plain_bits=pb, sec128=False)
    assert g.moduli == o.moduli and g.t == o.t
    sk = pk = None
    if keys:
        sk = o.keygen_secret(21)
        pk = o.keygen_public(sk, 22)
        g.set_secret_key(sk)
        g.set_public_key(pk)
    return g, o, N, sk, pk


def rand_cts(o, rng, n, L, size=2):
    return np.stack([o.random_poly(rng, L, size) for _ in range(n)])


def plains(o, rng, n, N):
    """n plaintexts mod t: a monomial, zero, -X^k, then full-range ones"""
    t = o.t
    m = rng.integers(0, t, (n, N), dtype=np.uint64)
    if n > 0:
        m[0] = 0
        m[0, 5] = 1
    if n > 1:
        m[1] = 0
    if n > 3:
        m[3] = 0
        m[3, N - 1] = t - 1
    return m


def lift(o, m, L):
    t = o.t
    c = np.where(m < np.uint64((t + 1) // 2), m.astype(object), m.astype(object) - t)
    return [(c % q).astype(np.uint64) for q in o.moduli[:L]]


def refused(be, f):
    with pytest.raises(be.HE355Error) as ei:
        f()
    assert ei.value.code == be.E_INVALID_ARGS, ei.value
    assert len(str(ei.value)) > len("he355 error 1: "), "a message goes with the code"
