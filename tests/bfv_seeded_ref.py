"""The definition of seeded BFV queries and Galois keys (include/he355.h "seeded BFV queries and Galois keys") in numpy uint64 and Python
integers: the counter-based sampler restated (csrc/client/sampler.h: splitmix64, the word of a coefficient, the uniform draw with its
rejection loop over the sub-counters 8n .. 8n + 7 and its fallback to the eighth draw, the centred binomial error), the stream functions, the
seeded zero, encryption, the selector c0, restoration in both forms and the halves of a seeded Galois key.  No device, no library code; the
oracle is read only for its transforms (ntt / intt) and, for the permuted key, apply_galois_poly.  test_bfv_seeded_ref_cpu.py holds the
restated sampler to sampler.h itself."""
import numpy as np

import bfv_selector_ref as selr

MAX_INDEX = 1 << 40
M64 = (1 << 64) - 1
_U = np.uint64


# ---- the sampler, restated ------------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def base(seed, stream):
    """sample_word(seed, stream, n) = splitmix64(base + n)"""
    return splitmix64(_U(seed) ^ splitmix64(_U(stream)))


def words(seed, stream, ns):
    with np.errstate(over="ignore"):
        return splitmix64(base(seed, stream) + np.asarray(ns, dtype=np.uint64))


def limit(q):
    """the largest accepted draw: one below the largest multiple of q that fits 64 bits"""
    return M64 - (M64 % q) - 1


def uniform_draws(seed, stream, ns, q):
    """(v, draws): the accepted 64-bit draw of every coefficient of `ns` and how many draws it took (1..8; 8 also when all eight were
    rejected: the eighth is kept)"""
    ns = np.asarray(ns, dtype=np.uint64)
    lim = _U(limit(q))
    with np.errstate(over="ignore"):
        v = words(seed, stream, _U(8) * ns)
        draws = np.ones(ns.shape, dtype=np.int32)
        for k in range(1, 8):
            again = v > lim
            if not again.any():
                break
            v[again] = words(seed, stream, _U(8) * ns[again] + _U(k))
            draws[again] = k + 1
    return v, draws


def uniform(seed, stream, N, q):
    """sample_uniform_at(seed, stream, n, q) for n < N"""
    v, _ = uniform_draws(seed, stream, np.arange(N, dtype=np.uint64), q)
    return v % _U(q)


def second_draws(seed, stream, N, q):
    """the coefficients n < N whose first draw was rejected"""
    _, d = uniform_draws(seed, stream, np.arange(N, dtype=np.uint64), q)
    return np.nonzero(d > 1)[0]


def _unsplitmix64(z):
    """the inverse of splitmix64 in Python integers: every step of it is a bijection of 64-bit words"""
    z = z ^ (z >> 31) ^ (z >> 62)
    z = z * pow(0x94D049BB133111EB, -1, 1 << 64) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & M64
    z = z ^ (z >> 30) ^ (z >> 60)
    return (z - 0x9E3779B97F4A7C15) & M64


def seed_with_second_draw(stream, n, q, salt=0):
    """a seed under which coefficient n of `stream` has its first draw rejected under q (probability 2^-25 .. 2^-46 per coefficient for the
    chains' primes: no search finds one, the inverse of splitmix64 does): the first draw is made M64 - salt, which lies above every limit"""
    first = M64 - salt
    assert first > limit(q)
    b = (_unsplitmix64(first) - 8 * n) & M64
    seed = _unsplitmix64(b) ^ int(splitmix64(_U(stream)))
    assert int(words(seed, stream, [8 * n])[0]) == first
    return seed


def _popcount21(v):
    c = np.zeros(v.shape, dtype=np.int32)
    for k in range(21):
        c += ((v >> _U(k)) & _U(1)).astype(np.int32)
    return c


def cbd(seed, stream, N):
    """sample_cbd_at(seed, stream, n) for n < N: popcount of bits 0..20 minus popcount of bits 21..41"""
    w = words(seed, stream, np.arange(N, dtype=np.uint64))
    return _popcount21(w) - _popcount21(w >> _U(21))


# ---- the streams ----------------------------------------------------------------------------------------------------------------------------
def a_stream(r, i):
    assert 0 <= r < MAX_INDEX and 0 <= i < 63
    return (1 << 48) + 64 * r + i


def e_stream(r):
    assert 0 <= r < MAX_INDEX
    return (1 << 48) + 64 * r + 63


def enc_stream(r, which):
    return 3 * r + which


def keygen_stream(key_id, digit, K, which):
    return (1 << 40) + (key_id * 64 + digit) * (K + 1) + which


# ---- ciphertexts -----------------------------------------------------------------------------------------------------------------------------
def a_hat(o, L, a_seed, index):
    """[L][N]: the seeded half of seeded ciphertext `index`, NTT form"""
    return np.stack([uniform(a_seed, a_stream(index, i), o.N, o.moduli[i]) for i in range(L)])


def error(o, noise_seed, index):
    return cbd(noise_seed, e_stream(index), o.N)


def _mod(x, q):
    return (x % q).astype(np.uint64)


def seeded_zero(o, sk, L, a_seed, noise_seed, index):
    """(c0, c1), [L][N] each, coefficient form: c0_i = -e - iNTT_i(a_i (.) s_i), c1_i = iNTT_i(a_i)"""
    assert a_seed != noise_seed
    a = a_hat(o, L, a_seed, index)
    e = error(o, noise_seed, index).astype(object)
    c0, c1 = [], []
    for i in range(L):
        q = o.moduli[i]
        w = o.intt(i, _mod(a[i].astype(object) * sk[i].astype(object), q)).astype(object)
        c0.append(_mod(-e - w, q))
        c1.append(o.intt(i, a[i]))
    return np.stack(c0), np.stack(c1)


def delta(o, L, m):
    """[L][N]: Delta_L(m) = floor((q_L m + floor((t + 1) / 2)) / t) mod q_i, q_L the product of the first L primes"""
    t, Q = o.t, 1
    for q in o.moduli[:L]:
        Q *= q
    d = (Q * np.asarray(m).astype(object) + (t + 1) // 2) // t
    return np.stack([_mod(d, q) for q in o.moduli[:L]])


def encrypt(o, sk, L, plain, a_seed, noise_seed, first_index):
    """plain [n][N] mod t (None: n = 1 zero) -> c0 [n][L][N]"""
    out = []
    for r in range(len(plain)):
        c0, _ = seeded_zero(o, sk, L, a_seed, noise_seed, first_index + r)
        d = delta(o, L, plain[r])
        out.append(np.stack([_mod(c0[i].astype(object) + d[i].astype(object), o.moduli[i]) for i in range(L)]))
    return np.stack(out)


def selector_c0(o, sk, L, v, sel, first_slot, count, a_seed, noise_seed, first_index):
    """sel [n][n_sel] mod t -> c0 [n][L][N]: the seeded zeros plus the plants of he355_bfv_selector_encrypt, polynomial 0"""
    n, n_sel = sel.shape
    d = selr.depth(count)
    where = selr.slots(o.moduli[:L], v, n_sel, first_slot)
    assert all(e < count <= o.N for e, *_ in where)
    out = []
    for r in range(n):
        c0, _ = seeded_zero(o, sk, L, a_seed, noise_seed, first_index + r)
        for e, b, i, g in where:
            q = o.moduli[i]
            c0[i, e] = (int(c0[i, e]) + selr.value(int(sel[r, b]), o.t, g, v, d, q)) % q
        out.append(c0)
    return np.stack(out)


def restore(o, L, ntt_form, c0, a_seed, first_index):
    """c0 [n][L][N] -> [n][2][L][N]"""
    out = np.empty((len(c0), 2, L, o.N), dtype=np.uint64)
    for r in range(len(c0)):
        a = a_hat(o, L, a_seed, first_index + r)
        for i in range(L):
            out[r, 0, i] = o.ntt(i, c0[r, i]) if ntt_form else c0[r, i]
            out[r, 1, i] = a[i] if ntt_form else o.intt(i, a[i])
    return out


# ---- Galois keys -----------------------------------------------------------------------------------------------------------------------------
def galois_key(o, sk, elt, a_seed, noise_seed):
    """(b, a), [L_top][K][N] each, NTT form: digit j, prime i: a from a_seed's keygen_stream(2 + elt, j, K, i), e from noise_seed's
    keygen_stream(2 + elt, j, K, K), b = -(a s + NTT(e)) + [i == j] (P mod q_j) s(X^elt).  Equal seeds are he355_keygen_galois's key."""
    K, Lt, N = len(o.moduli), len(o.moduli) - 1, o.N
    P = o.moduli[K - 1]
    b = np.empty((Lt, K, N), dtype=np.uint64)
    a = np.empty((Lt, K, N), dtype=np.uint64)
    for j in range(Lt):
        e = cbd(noise_seed, keygen_stream(2 + elt, j, K, K), N).astype(object)
        for i in range(K):
            q = o.moduli[i]
            a[j, i] = uniform(a_seed, keygen_stream(2 + elt, j, K, i), N, q)
            v = -(a[j, i].astype(object) * sk[i].astype(object) + o.ntt(i, _mod(e, q)).astype(object))
            if i == j:
                v = v + (P % q) * o.apply_galois_poly(i, elt, True, sk[i]).astype(object)
            b[j, i] = _mod(v, q)
    return b, a


def full_key(b, a):
    """[L_top][2][K][N], what he355_set_galois_key takes"""
    return np.stack([b, a], axis=1)
