"""What the tests of the BFV monomial multiply and the query expansion share (test_gpu_bfv_expand.py, test_gpu_bfv_large_rings.py): the numpy
negacyclic shift and the expansion tree by its definition, run in the oracle.  numpy and the oracle only."""
import numpy as np


def np_shift(x, e, moduli):
    """x X^e mod (X^N + 1, q_i) for x [..., L, N] uint64 canonical residues, e in [0, 2N): numpy, the negative of 0 is 0"""
    N = x.shape[-1]
    assert 0 <= e < 2 * N
    r = e % N
    out = np.roll(x, r, axis=-1)
    flip = (np.arange(N) < r) ^ (e >= N)  # wrapped past X^N once, and once more for e >= N
    for i in range(x.shape[-2]):
        q = np.uint64(moduli[i])
        v = out[..., i, :]
        out[..., i, :] = np.where(flip & (v != 0), q - v, v)
    return out


def expand_levels(o, c, d, gks, L):
    """levels[j] = the 2^j nodes after j levels of the definition, for one query c [2][L][N]"""
    N = o.N
    levels = [[c]]
    for j in range(d):
        s, e = 1 << j, N // (1 << j) + 1
        new = [None] * (2 * s)
        for k, node in enumerate(levels[-1]):
            gal = o.apply_galois(node, e, gks[e])
            new[k] = o.add(node, gal)
            new[k + s] = np_shift(o.sub(node, gal), 2 * N - s, o.moduli)
        levels.append(new)
    return levels


def children(levels, count):
    """the `count` children of one query: a cut last level computes the same values, fewer of them"""
    d = (count - 1).bit_length()
    return levels[d][:count]
