"""References of the fused BFV PIR calls that use no device (test_bfv_ring_ref_cpu.py holds them to Python integers, test_gpu_bfv_large_rings.py
holds the device to them): numpy for the cuts (bfv_gadget_ref.np_digits / np_spread, bfv_bytes_ref.np_fields, the centred lift) and the oracle
for every transform and every product (oracle.Context.ntt / intt, multiply_ntt with a zero second polynomial as the pointwise product, add).
All of it is exact: canonical residues in, canonical residues out."""
import numpy as np

import bfv_gadget_ref as gad
import bfv_selector_ref as sel
from bfv_bytes_ref import np_fields


def np_lift(m, t, q):
    """bfv_gadget_ref.lift under one prime, vectorised: m below floor((t + 1) / 2) as is, else m - t, both mod q (m < t < 2^32; q may
    lie below t: the chains of tests/explicit_moduli.py)"""
    m = np.asarray(m, dtype=np.uint64)
    r = m % np.uint64(q)
    return np.where(m < np.uint64((t + 1) // 2), r, (r + np.uint64(q - t % q)) % np.uint64(q))


def ntt_all(o, x):
    """o.ntt of every polynomial of [..][L][N], prime i at index i of the second-to-last axis"""
    out = np.empty_like(x)
    L, N = x.shape[-2:]
    flat, dst = x.reshape(-1, L, N), out.reshape(-1, L, N)
    for p in range(flat.shape[0]):
        for i in range(L):
            dst[p, i] = o.ntt(i, flat[p, i])
    return out


def intt_all(o, x):
    out = np.empty_like(x)
    L, N = x.shape[-2:]
    flat, dst = x.reshape(-1, L, N), out.reshape(-1, L, N)
    for p in range(flat.shape[0]):
        for i in range(L):
            dst[p, i] = o.intt(i, flat[p, i])
    return out


def lifted_ntt(o, m, L_out):
    """[..][N] coefficients below t -> [..][L_out][N]: the centred lift under each prime i' < L_out, then o.ntt"""
    return ntt_all(o, np.stack([np_lift(m, o.t, q) for q in o.moduli[:L_out]], axis=-2))


def decompose_ntt_ref(o, x, L_out):
    """he355_bfv_decompose_ntt: x [n][size][L][N] -> [n][size D(L)][L_out][N], digits of width bitlen(t) - 1"""
    return lifted_ntt(o, gad.np_digits(x, o.moduli, o.t.bit_length() - 1), L_out)


def unpack_bytes_ntt_ref(o, data, L_out):
    """he355_bfv_unpack_bytes_ntt: data [n][B] uint8 -> [n][L_out][N], fields of width bitlen(t) - 1"""
    return lifted_ntt(o, np_fields(data, o.t.bit_length() - 1, o.N), L_out)


def gadget_ntt_ref(o, x, v):
    """he355_bfv_gadget_decompose_ntt: x [n][size][L][N] -> [n][size E(L)][L][N], the plain digits of width v under every prime"""
    L = x.shape[2]
    return ntt_all(o, gad.np_spread(gad.np_digits(x, o.moduli, v), o.moduli[:L]))


def mac_ntt(o, rows, digits):
    """sum over terms of rows [T][2][L][N] (NTT form) (.) digits [T][L][N] (NTT form) -> [2][L][N], NTT form.  multiply_ntt of (r0, r1) and
    (d, 0) leaves (r0 d, r1 d, 0): the pointwise product of both polynomials under every prime; oracle.add sums them"""
    T, _, L, N = rows.shape
    assert digits.shape == (T, L, N)
    acc = np.zeros((2, L, N), dtype=np.uint64)
    d = np.zeros((2, L, N), dtype=np.uint64)
    for k in range(T):
        d[0] = digits[k]
        acc = o.add(acc, o.multiply_ntt(np.ascontiguousarray(rows[k]), d)[:2])
    return acc


def external_product_ref(o, cts, rgsw, v, digits=None):
    """one result of he355_bfv_external_product: cts [inner][2][L][N] (coefficient form), rgsw [inner][2E][2][L][N] (NTT form) ->
    [2][L][N], coefficient form.  Term (kappa, f) is RGSW row f of selector kappa against digit polynomial f of ciphertext kappa.
    digits: gadget_ntt_ref(o, cts, v) where the caller has it already (results that share ciphertexts)"""
    inner, _, L, N = cts.shape
    if digits is None:
        digits = gadget_ntt_ref(o, cts, v)
    rows = digits.shape[1]
    assert rgsw.shape == (inner, rows, 2, L, N)
    return intt_all(o, mac_ntt(o, rgsw.reshape(inner * rows, 2, L, N), digits.reshape(inner * rows, L, N)))


def rgsw_from_bfv_rows(o, ct, key, kv):
    """one slot ciphertext ct [2][L][N] (coefficient form), key [2 E_key][2][L][N] (NTT form) -> (row k = 0, row k = 1), NTT form: its own
    transform, and the sums of its key_bits digits against the key rows with no inverse transform"""
    L, N = ct.shape[1:]
    digits = gadget_ntt_ref(o, ct[None], kv)[0]
    assert key.shape == (digits.shape[0], 2, L, N)
    return ntt_all(o, ct), mac_ntt(o, key, digits)


def rgsw_from_bfv_ref(o, slots, key, v, kv):
    """he355_bfv_rgsw_from_bfv: slots [C][2][L][N] in slot order c = (r n_sel + b) E + f -> [C / E][2E][2][L][N] by bfv_selector_ref's row rule"""
    L = slots.shape[2]
    E = gad.table(o.moduli[:L], v)[1][-1]
    k0, k1 = zip(*(rgsw_from_bfv_rows(o, c, key, kv) for c in slots))
    return sel.np_rows(np.stack(k0), np.stack(k1), E)
