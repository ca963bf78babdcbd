"""What the tests of the BFV external product share (test_bfv_gadget_core_cpu.py, test_gpu_bfv_external_product.py): the gadget table of a
digit width v, the numpy digit cut (plain non-negative integers, no centred lift), the gadget identity, the planted value of an RGSW row and
the negacyclic product by a sparse polynomial in Z_t[X]/(X^N + 1).  Python integers and numpy only."""
import numpy as np


def table(moduli, v):
    """(E_i per prime, off_i with off[L] = E(L)) for digit width v"""
    E = [-(-q.bit_length() // v) for q in moduli]
    return E, [sum(E[:i]) for i in range(len(moduli) + 1)]


def digit(x, g, v):
    return (x >> (g * v)) & ((1 << v) - 1)


def gadget(moduli, v):
    """the gadget elements in digit order: G_(i,g) as its RNS residues, 2^(g v) mod q_i under prime i and 0 elsewhere"""
    E, _ = table(moduli, v)
    return [[(1 << (g * v)) % q if j == i else 0 for j, q in enumerate(moduli)] for i in range(len(moduli)) for g in range(E[i])]


def identity_holds(x, moduli, v):
    """x: canonical RNS residues of one value.  sum_(i,g) digit_(i,g)(x_i) G_(i,g) == x under every prime, i.e. mod q_L"""
    E, _ = table(moduli, v)
    digits = [digit(x[i], g, v) for i in range(len(moduli)) for g in range(E[i])]
    G = gadget(moduli, v)
    return all(sum(d * Gf[j] for d, Gf in zip(digits, G)) % q == x[j] for j, q in enumerate(moduli))


def np_digits(x, moduli, v):
    """[n][size][L][N] canonical residues -> [n][size E(L)][N] plain digits, polynomial k, prime i, digit g at k E(L) + off_i + g"""
    n, size, L, N = x.shape
    E, off = table(moduli[:L], v)
    out = np.empty((n, size, off[-1], N), dtype=np.uint64)
    mask = np.uint64((1 << v) - 1)
    for i in range(L):
        for g in range(E[i]):
            out[:, :, off[i] + g, :] = (x[:, :, i, :] >> np.uint64(g * v)) & mask
    return out.reshape(n, size * off[-1], N)


def np_spread(d, moduli):
    """[..][N] digits -> [..][L][N]: the same integers under every prime, reduced where they are not below it"""
    return np.stack([d % np.uint64(q) for q in moduli], axis=-2)


def lift(m, t):
    """the centred lift of he355_bfv_multiply_plain: m below floor((t + 1) / 2) as is, else m - t"""
    return m if m < (t + 1) // 2 else m - t


def plant(m, t, g, v, q):
    return lift(m, t) * (1 << (g * v)) % q


def np_plant(zero, m, moduli, t, v):
    """zero [2E][2][L][N] (rows of one RGSW: encryptions of zero cut to L primes, coefficient form), m [N] mod t -> the rows with
    lift(m) 2^(g v) mod q_i added to polynomial k under prime i of row k E + off_i + g"""
    rows, _, L, N = zero.shape
    E, off = table(moduli[:L], v)
    assert rows == 2 * off[-1]
    out = zero.copy()
    lifted = np.array([lift(int(c), t) for c in m], dtype=object)
    for k in range(2):
        for i, q in enumerate(moduli[:L]):
            for g in range(E[i]):
                f = k * off[-1] + off[i] + g
                add = ((lifted << (g * v)) % q).astype(np.uint64)
                s = out[f, k, i].astype(object) + add.astype(object)
                out[f, k, i] = (s % q).astype(np.uint64)
    return out


def negacyclic_sparse(mu, sparse, t):
    """mu [N] mod t times the sparse polynomial {exponent: coefficient mod t} in Z_t[X]/(X^N + 1), Python integers"""
    N = len(mu)
    a = [int(c) for c in mu]
    out = [0] * N
    for e, c in sparse.items():
        c %= t
        if not c:
            continue
        for i in range(N):
            k = i + e
            if k < N:
                out[k] = (out[k] + c * a[i]) % t
            else:
                out[k - N] = (out[k - N] - c * a[i]) % t
    return np.array(out, dtype=np.uint64)
