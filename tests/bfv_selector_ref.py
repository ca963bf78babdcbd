"""What the tests of the packed RGSW selectors share (test_bfv_selector_core_cpu.py, test_gpu_bfv_selectors.py), beside bfv_gadget_ref.py: the
depth of an expansion, the value a selector plants, the numpy packing of he355_bfv_selector_encrypt, the by-hand reading of one expanded slot
and the row layout of he355_bfv_rgsw_from_bfv.  Python integers and numpy only."""
import numpy as np

import bfv_gadget_ref as gad


def depth(count):
    """d = ceil(log2 count), the levels of he355_bfv_expand(.., count, ..)"""
    return (count - 1).bit_length()


def value(m, t, g, v, d, q):
    """lift(m) 2^(g v) (2^d)^(-1) mod q"""
    return gad.lift(m, t) * (1 << (g * v)) * pow(1 << d, -1, q) % q


def slots(moduli, v, n_sel, first_slot):
    """[(coefficient, selector b, prime i, digit g)] in slot order: coefficient first_slot + b E + off_i + g"""
    E, off = gad.table(moduli, v)
    return [(first_slot + b * off[-1] + off[i] + g, b, i, g) for b in range(n_sel) for i in range(len(moduli)) for g in range(E[i])]


def np_pack(zero, sel, moduli, t, v, first_slot, count):
    """zero [n][2][L][N] (encryptions of zero cut to L primes, coefficient form), sel [n][n_sel] mod t -> the query ciphertexts: polynomial 0
    under prime i ONLY receives value(m_(r,b)) at the coefficient of slot (b, i, g)"""
    n, _, L, N = zero.shape
    d = depth(count)
    out = zero.copy()
    where = slots(moduli[:L], v, sel.shape[1], first_slot)
    assert all(e < count <= N for e, *_ in where)
    for r in range(n):
        for e, b, i, g in where:
            q = moduli[i]
            out[r, 0, i, e] = (int(out[r, 0, i, e]) + value(int(sel[r, b]), t, g, v, d, q)) % q
    return out


def expanded_constant(poly, slot, d, q):
    """what child `slot` of an expansion of depth d holds at X^0, for a query polynomial supported below 2^d: 2^d times coefficient `slot`"""
    assert len(poly) >= 1 << d > slot
    return (1 << d) * int(poly[slot]) % q


def row(c, E, k):
    """slot ciphertext c = (selector) E + f -> its row of the slab [.][2E][2][L][N]: k = 0 its own transform, k = 1 its product with RGSW(s)"""
    return (c // E) * 2 * E + k * E + c % E


def np_rows(k0, k1, E):
    """k0, k1 [C][2][L][N] (the rows of slot ciphertext c, C a multiple of E) -> [C / E][2E][2][L][N]"""
    C = k0.shape[0]
    assert C % E == 0 and k1.shape == k0.shape
    out = np.empty((2 * C,) + k0.shape[1:], dtype=np.uint64)
    for c in range(C):
        out[row(c, E, 0)] = k0[c]
        out[row(c, E, 1)] = k1[c]
    return out.reshape((C // E, 2 * E) + k0.shape[1:])
