"""The definition of BFV reply compression (include/he355.h, csrc/bfv_reply_core.h) in Python integers: the switch to 2^k, the bit layout,
the client's decryption and its budget.  No device, no library code.  The numpy helpers at the end are the same definition on arrays, for
the GPU tests; test_bfv_reply_ref_cpu.py holds them to the integer functions."""
import numpy as np


# ---- widths and sizes ---------------------------------------------------------------------------------------------------------------------
def accepted(N, q, k0, k1):
    return 2 <= k0 <= k1 and N * 2 ** (k1 - 1) <= (q - 1) // 2


def max_width(N, q):
    """the largest accepted k1"""
    k = 2
    while accepted(N, q, 2, k + 1):
        k += 1
    return k


def safe_bits(N, t):
    k0 = t.bit_length() + 2
    return k0, k0 + N.bit_length() - 1


def reply_bytes(N, k0, k1):
    return N * (k0 + k1) // 8


def check_widths(N, q, k0, k1):
    if not accepted(N, q, k0, k1):
        raise ValueError(f"widths ({k0}, {k1}) are refused at N = {N}, q = {q}")


# ---- the switch -----------------------------------------------------------------------------------------------------------------------------
def cut(x, k, q):
    assert 0 <= x < q
    return ((x * 2 ** k + q // 2) // q) % 2 ** k


# ---- the layout -------------------------------------------------------------------------------------------------------------------------------
def pack(y0, y1, k0, k1):
    """the reply's bytes: c0's fields of k0 bits, then c1's fields of k1 bits, coefficient e at bit e k"""
    N = len(y0)
    v = 0
    for e in range(N):
        assert 0 <= y0[e] < 2 ** k0 and 0 <= y1[e] < 2 ** k1
        v |= int(y0[e]) << (e * k0)
        v |= int(y1[e]) << (N * k0 + e * k1)
    return v.to_bytes(reply_bytes(N, k0, k1), "little")


def unpack(data, N, k0, k1):
    assert len(data) == reply_bytes(N, k0, k1)
    v = int.from_bytes(data, "little")
    y0 = [(v >> (e * k0)) & (2 ** k0 - 1) for e in range(N)]
    y1 = [(v >> (N * k0 + e * k1)) & (2 ** k1 - 1) for e in range(N)]
    return y0, y1


def compress(c0, c1, q, k0, k1):
    check_widths(len(c0), q, k0, k1)
    return pack([cut(int(x), k0, q) for x in c0], [cut(int(x), k1, q) for x in c1], k0, k1)


# ---- decryption -------------------------------------------------------------------------------------------------------------------------------
def centre(y, k):
    return y - 2 ** k if y >= 2 ** (k - 1) else y


def centred_mod(x, q):
    r = x % q
    return r - q if r > q // 2 else r


def negacyclic(a, s):
    """the integer product a s mod X^N + 1 (Python integers; s sparse or small is fast enough at N = 1024)"""
    N = len(a)
    a = np.array([int(x) for x in a], dtype=object)
    acc = np.zeros(N, dtype=object)
    for i, si in enumerate(s):
        si = int(si)
        if si:
            acc += si * np.concatenate((-a[N - i:], a[:N - i]))  # X^i a: the top i coefficients wrap with a sign
    return [int(x) for x in acc]


def finish(y0, w, k0, k1, t):
    """(plaintext coefficients, r): w the centred product, r the largest |t z - M 2^k1|"""
    plain, r = [], 0
    for a, b in zip(y0, w):
        z = (int(a) * 2 ** (k1 - k0) + int(b)) % 2 ** k1
        M = (t * z + 2 ** (k1 - 1)) // 2 ** k1
        r = max(r, abs(t * z - M * 2 ** k1))
        plain.append(M % t)
    return plain, r


def budget_of(k1, r):
    """(budget, noise_bits)"""
    nb = int(r).bit_length()
    return max(0, k1 - nb - 1), nb


def decrypt(data, N, k0, k1, q, t, s):
    """(plain, budget, noise_bits) of one reply under the secret key s (coefficients, any integers)"""
    check_widths(N, q, k0, k1)
    y0, y1 = unpack(data, N, k0, k1)
    w = [centred_mod(x, q) for x in negacyclic([centre(y, k1) for y in y1], s)]
    plain, r = finish(y0, w, k0, k1, t)
    return (plain,) + budget_of(k1, r)


# ---- the same on numpy arrays (the GPU tests) ---------------------------------------------------------------------------------------------------
def np_cut(x, k, q):
    """x: uint64 array of residues mod q -> uint64"""
    v = (x.astype(object) * 2 ** k + q // 2) // q % 2 ** k
    return v.astype(np.uint64)


def np_pack_half(y, k):
    """[n][N] fields of k bits -> [n][N k / 8] bytes"""
    n, N = y.shape
    bits = ((y[:, :, None] >> np.arange(k, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(n, N * k), axis=1, bitorder="little")


def np_compress(ct, q, k0, k1):
    """ct [n][2][1][N] (or [n][2][N]) at L = 1 -> [n][reply bytes] uint8"""
    n, N = ct.shape[0], ct.shape[-1]
    check_widths(N, q, k0, k1)
    c = ct.reshape(n, 2, N)
    return np.concatenate((np_pack_half(np_cut(c[:, 0], k0, q), k0), np_pack_half(np_cut(c[:, 1], k1, q), k1)), axis=1)


def np_fields(data, k, N):
    """[n][N k / 8] bytes -> [n][N] fields"""
    n = data.shape[0]
    bits = np.unpackbits(data, axis=1, bitorder="little").reshape(n, N, k).astype(np.uint64)
    return (bits << np.arange(k, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def np_unpack(data, N, k0, k1):
    """[n][reply bytes] uint8 -> (y0, y1) [n][N] uint64"""
    cutoff = N * k0 // 8
    return np_fields(data[:, :cutoff], k0, N), np_fields(data[:, cutoff:], k1, N)


def np_lift(y1, k1, q):
    """y1 centred, as residues mod q (uint64)"""
    c = y1.astype(object)
    c = np.where(y1 >= np.uint64(2 ** (k1 - 1)), c - 2 ** k1, c)
    return (c % q).astype(np.uint64)


def np_finish(y0, w, k0, k1, q, t):
    """y0 [n][N] fields, w [n][N] the product's residues mod q -> (plain [n][N] uint64, budget [n], noise_bits [n])"""
    wc = w.astype(object)
    wc = np.where(w > np.uint64(q // 2), wc - q, wc)
    z = (y0.astype(object) * 2 ** (k1 - k0) + wc) % 2 ** k1
    M = (t * z + 2 ** (k1 - 1)) // 2 ** k1
    res = abs(t * z - M * 2 ** k1)
    pairs = [budget_of(k1, max(row)) for row in res]
    return (M % t).astype(np.uint64), np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32)
