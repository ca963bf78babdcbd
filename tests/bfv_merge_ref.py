"""What the tests of the BFV ciphertext merge share (test_bfv_merge_ref_cpu.py, test_gpu_bfv_merge.py): the merge by its definition, run in
the oracle (oracle.add / oracle.sub / oracle.apply_galois and the numpy shift of bfv_expand_ref), and the closed form of what it decrypts
to.  numpy and the oracle only."""
import numpy as np

from bfv_expand_ref import np_shift


def merge_levels(o, cts, count, gks, L):
    """the one ciphertext [2][L][N] the `count` ciphertexts cts[k] merge into: for j = d-1 .. 0, s = 2^j, slot k < s becomes
    S + galois(D, N / 2^j + 1) with S = even + X^s odd, D = even - X^s odd (S = D = even where slot k + s is absent)"""
    assert len(cts) == count and all(c.shape[1] == L for c in cts)
    N = o.N
    d = (count - 1).bit_length()
    slots = list(cts)
    for j in range(d - 1, -1, -1):
        s, e = 1 << j, N // (1 << j) + 1
        new = []
        for k in range(s):
            even = slots[k]
            if k + s < len(slots):
                odd = np_shift(slots[k + s], s, o.moduli)
                S, D = o.add(even, odd), o.sub(even, odd)
            else:
                S = D = even
            new.append(o.add(S, o.apply_galois(D, e, gks[e])))
        slots = new
    return slots[0].copy()


def merged_plain(mu, t):
    """what the merge of inputs decrypting to mu [count][N] decrypts to: coefficient k + 2^d m is 2^d mu[k, 2^d m] mod t, 0 for the absent k"""
    count, N = mu.shape
    d = (count - 1).bit_length()
    want = np.zeros(N, dtype=np.uint64)
    for k in range(count):
        want[k::1 << d] = (mu[k, ::1 << d].astype(object) * (1 << d) % t).astype(np.uint64)
    return want


def decrypt(o, sk, ct):
    return o.bfv_decode_phase(o.decrypt_phase(ct, sk))
