"""The definition of he355_ckks_mod_raise and he355_ckks_lift_centred, with no device (include/he355.h writes it out): the transforms are the
oracle's (bfv_ring_ref.ntt_all / intt_all: oracle.Context.ntt / intt), the lift is done in Python integers.

    x   = iNTT_{q_0}(in[p][0])
    c_e = x_e if x_e <= (q_0 - 1) / 2 else x_e - q_0
    out[p][j] = NTT_{q_j}(c mod q_j),  j < L_to

tests/test_ckks_mod_raise_ref_cpu.py holds it to exact integers (CRT, tie points, the decryption identity); tests/test_gpu_ckks_mod_raise.py holds
the device to it bit for bit.  Also here: the coefficient patterns both tests use and the restated rule of the small-batch split."""
import numpy as np

from bfv_ring_ref import intt_all, ntt_all


def centred(x, q0):
    """[..] canonical residues under q_0 -> Python integers in [-(q_0 - 1) / 2, (q_0 - 1) / 2] (object array)"""
    x = np.asarray(x, dtype=np.uint64).astype(object)
    return np.where(x <= (q0 - 1) // 2, x, x - q0)


def lift_centred(moduli, coeff, L_to):
    """he355_ckks_lift_centred: coeff [..][N] canonical under moduli[0] -> [..][L_to][N], row j = c mod q_j (coefficient form)"""
    c = centred(coeff, moduli[0])
    return np.stack([(c % q).astype(np.uint64) for q in moduli[:L_to]], axis=-2)


def mod_raise(o, x, L_to):
    """he355_ckks_mod_raise: x [..][L_in][N], NTT form (only row 0 is read) -> [..][L_to][N], NTT form"""
    row0 = np.ascontiguousarray(x[..., :1, :])
    coeff = intt_all(o, row0)[..., 0, :]
    out = ntt_all(o, lift_centred(o.moduli, coeff, L_to))
    assert np.array_equal(out[..., 0, :], row0[..., 0, :])  # NTT(iNTT(row 0)) is row 0: the device makes it by a copy
    return out


def tsplit_rule(polys, L_to, cus):
    """the targets of a column are dealt to this many blocks: with polys * 4 blocks below the compute-unit count,
    min(L_to - 1, ceil(CUs / (polys * 4))); else 1"""
    blocks = polys * 4
    if L_to < 3 or blocks >= cus:
        return 1
    return min(L_to - 1, -(-cus // blocks))


def edge_operands(q0, qj):
    """the operands of the core test under one (q_0, q_j) pair: 0, 1, q_0 - 1, both tie points, and |c| = q_j, 2 q_j, the largest multiple
    of q_j below q_0 / 2 and their neighbours, on both signs (canonical residues under q_0, deduplicated, in range)"""
    half = (q0 - 1) // 2
    mags = {0, 1, half, half - 1}
    top = (half // qj) * qj
    for m in (qj, 2 * qj, top):
        mags |= {m - 1, m, m + 1}
    out = set()
    for m in mags:
        if 0 <= m <= half:
            out |= {m, (q0 - m) % q0}
    out |= {q0 - 1, half, half + 1}
    return sorted(out)


def patterns(moduli, N, rng):
    """{name: [N] coefficients canonical under q_0}: the coefficient patterns whose NTT images the device test raises"""
    q0 = moduli[0]
    half = (q0 - 1) // 2
    u = lambda v: np.full(N, v, dtype=np.uint64)
    pats = {"zero": u(0), "all_q0_minus_1": u(q0 - 1), "tie_low": u(half), "tie_high": u(half + 1)}
    alt = u(half)
    alt[1::2] = half + 1
    pats["alternating_ties"] = alt
    alt2 = u(1)
    alt2[1::2] = q0 - 1
    pats["alternating_signs"] = alt2
    imp = u(0)
    imp[N - 1] = q0 - 1
    pats["impulse"] = imp
    for j, qj in enumerate(moduli[1:], 1):
        ops = edge_operands(q0, qj)
        m = np.array([ops[e % len(ops)] for e in range(N)], dtype=np.uint64)
        pats[f"multiples_of_q{j}"] = m
    pats["uniform"] = rng.integers(0, q0, N, dtype=np.uint64)
    return pats
