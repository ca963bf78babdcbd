"""What the BFV GPU test modules (test_gpu_bfv_*.py) share: the parameter chains, the `be` fixture (imported by name), the device / oracle
context pair with its keys and expansion keys, random and edged operands, the sentinel convention around an output (sentinelled / inner_of,
`At` a slab offset), the route counters, the raw-allocation comparison, the external product's definition by composition, and the check of a
refused call."""
import importlib

import numpy as np
import pytest

from tools.probe_common import At  # noqa: F401 (the one definition, shared with the probes)

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
# the Shoup build of the u64 engine at LOGN1 = 4 (tests/shoup_rings.py, "n16384_60_50_40_60_shoup"): the level, NTT-form and noise calls
ALL["n16384_shoup"] = (16384, [60, 50, 40, 60], 20)

SENT = np.uint64(0x5E17155E17155E17)


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device")
    return mod


def pair(be, oracle, chain, keys=False):
    """(g, o, N, sk, pk): a device context and the oracle's of one chain -- a name of ALL, (N, bit sizes, plain bits) itself, or
    (N, primes, t) with the moduli themselves (told apart by size: no bit size passes 60, no admitted prime is below 12289); keys: the
    oracle's secret and public key, set on the device (else None)"""
    N, bits, pb = ALL[chain] if isinstance(chain, str) else chain
    if max(bits) > 60:
        g = be.Context(be.SCHEME_BFV, N, primes=list(bits), plain_modulus=pb, device=0)
        o = oracle.Context(oracle.SCHEME_BFV, N, primes=list(bits), plain_modulus=pb)
    else:
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


def expand_keys(g, o, sk, count, seed):
    """{elt: key}: the Galois keys of an expansion (or merge) of `count`, level j's from seed + j, set on the device"""
    gks = {}
    for j, e in enumerate(g.bfv_expand_galois_elts(count)):
        gks[e] = o.keygen_galois(sk, e, seed + j)
        g.set_galois_key(e, gks[e])
    return gks


def keyed(be, oracle, chain, count, seed):
    g, o, N, sk, pk = pair(be, oracle, chain, keys=True)
    return g, o, N, sk, pk, expand_keys(g, o, sk, count, seed)


def rand_cts(o, rng, n, L, size=2):
    return np.stack([o.random_poly(rng, L, size) for _ in range(n)])


def edged(o, rng, n, L, size=2):
    """uniform rows mixed with all-0, all-(q - 1) and alternating rows"""
    c = rand_cts(o, rng, n, L, size)
    c[0, 0, 0, :] = 0
    for i, q in enumerate(o.moduli[:L]):
        c[n - 1, size - 1, i, :] = q - 1
        c[1 % n, 0, i, 1::2] = 0
        c[1 % n, 0, i, 0::2] = q - 1
    return c


def to_level(o, ct, L):
    while ct.shape[1] > L:
        ct = o.mod_switch_coeff(ct)
    return ct


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


def sentinelled(g, words, N):
    return g.to_device(np.full(words + 2 * N, SENT, dtype=np.uint64))


def inner_of(buf, N, what):
    got = buf.download()
    assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), (what, "sentinel")
    return got[N:-N]


def routes(g):
    """the counters of he355_bfv_route_stats that are not zero"""
    return {k: c for k, c in g.bfv_route_stats().items() if c}


def same_allocs(a, b):
    return (a["raw_mallocs"], a["raw_frees"]) == (b["raw_mallocs"], b["raw_frees"])


def ep_composition(g, L, v, n, inner, x, ct_at, rg, rg_stride_r, rows, N):
    """the external product's definition, per result: gadget_decompose_ntt of its inner ciphertexts (gathered on the host),
    multiply_plain_accumulate over the inner 2E terms with the RGSW rows as the ciphertext operand, transform_from_ntt.  x: the ciphertext
    slab on the host, ct_at(r, k) its index"""
    per = 2 * L * N
    out = np.empty((n, 2, L, N), dtype=np.uint64)
    dig, res = g.alloc(inner * rows * L * N), g.alloc(per)
    for r in range(n):
        cts = g.to_device(np.stack([x[ct_at(r, k)] for k in range(inner)]))
        g.bfv_gadget_decompose_ntt(L, v, 2, inner, cts, dig)
        g.bfv_multiply_plain_accumulate(L, 2, 1, 1, inner * rows, At(rg, r * rg_stride_r * rows * per), 1, 1, dig, 1, 1, res)
        g.bfv_transform_from_ntt(L, 2, 1, res, res)
        out[r] = res.download((2, L, N))
        cts.free()
    dig.free()
    res.free()
    return out
