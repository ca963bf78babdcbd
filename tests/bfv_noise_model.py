"""The reference model of the BFV invariant noise budget (SEAL v3.7.2 Decryptor::invariant_noise_budget) in Python integers, independent
of the product: used by tests/test_bfv_noise_core_cpu.py and tests/test_gpu_bfv_noise.py.

  phase (coefficient form, from oracle.Context.decrypt_phase) -> every residue times t mod q_i -> CRT-composed x in [0, q_L)
  -> |x| = q_L - x where x >= (q_L + 1) // 2 else x -> norm = max over the coefficients -> noise_bits = norm.bit_length()
  -> budget = max(0, q_L.bit_length() - noise_bits - 1)"""
import numpy as np


def q_product(qs):
    qL = 1
    for q in qs:
        qL *= int(q)
    return qL


def compose(res, qs):
    """res [L][n] canonical residues -> object array [n] of x in [0, q_L)"""
    qL = q_product(qs)
    x = np.zeros(res.shape[1], dtype=object)
    for i, q in enumerate(qs):
        q = int(q)
        p = qL // q
        x = x + res[i].astype(object) * (p * pow(p, -1, q))
    return x % qL


def noise_of_phase(phase, qs, t):
    """(noise_bits, budget, bits(q_L)) of a phase [L][N] under the primes qs"""
    qs = [int(q) for q in qs]
    qL = q_product(qs)
    scaled = np.stack([(phase[i].astype(object) * int(t)) % q for i, q in enumerate(qs)])
    norm = 0
    for x in compose(scaled, qs):
        x = int(x)
        norm = max(norm, qL - x if x >= (qL + 1) // 2 else x)
    nb = norm.bit_length()
    return nb, max(0, qL.bit_length() - nb - 1), qL.bit_length()


def noise_of(o, ct, sk):
    """(noise_bits, budget, bits(q_L)) of the ciphertext ct [size][L][N] (coefficient form) under the secret key sk [K][N], o: the oracle context"""
    L = ct.shape[1]
    return noise_of_phase(o.decrypt_phase(np.ascontiguousarray(ct), sk), o.moduli[:L], o.t)


def magnitude_bits(x, qL):
    """bit length of the centred magnitude of x in [0, q_L)"""
    return (qL - x if x >= (qL + 1) // 2 else x).bit_length()


def edge_values(qL):
    """the composed values the bit-length and centring code must get right: 0, 1, q_L - 1, the three around the centring threshold, and
    2^k - 1, 2^k, 2^k + 1 at every word boundary k (multiple of 64, k < bits(q_L) - 1) and at k = bits(q_L) - 2"""
    vals = [0, 1, qL - 1, (qL - 1) // 2, (qL + 1) // 2, (qL + 1) // 2 + 1]
    nb = qL.bit_length()
    ks = [k for k in range(64, nb - 1, 64)] + [nb - 2]
    for k in ks:
        vals += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    assert all(0 <= v < qL for v in vals)
    return vals


def residues_for(x, qs, t):
    """residues r_i with (r_i t mod q_i) composing to x: those of x t^-1 mod q_L"""
    qL = q_product(qs)
    y = (x * pow(int(t), -1, qL)) % qL
    return [y % int(q) for q in qs]
