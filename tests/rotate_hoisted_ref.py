"""The definition of the hoisted rotations (include/he355.h: he355_apply_galois_hoisted, he355_rotate_hoisted,
he355_rotate_hoisted_plain_sum) from oracle calls only.  For a size-2 ciphertext (c0, c1) at level L, element g with key key_g
[Ltop][2][K][N] and g^-1 its inverse mod 2N:

  1. key' = every residue polynomial of key_g permuted in NTT form by g^-1   (Context.apply_galois_poly(i, g^-1, 1, .))
  2. (u0, u1) = the ordinary key switch of c1 under key', added into (c0, 0)   (Context.switch_key(c1, key', (c0, 0)))
  3. out = sigma_g of both polynomials                                          (Context.apply_galois_poly(i, g, ntt_form, .))

g = 1 is the identity.  CKKS ciphertexts are in NTT form; a BFV context's are in coefficient form (ntt_form 0) or, for ntt_form 1, the
definition is ntt(ref_coeff(intt(x))).  The plain sum is the oracle's multiply_plain and add over the hoisted terms.  No GPU, no backend."""
import numpy as np

# CKKS: the slot error of a hoisted rotation is held to this many times the ordinary rotation's on the same ciphertext.  The two key
# switches add noise of the same bound (the digits differ by a sign convention the key absorbs); 1.46 x is the most that was measured, and a
# wrong key permutation or element gives errors of the size of the values themselves, 10^4 times the cap.
CKKS_ERROR_CAP = 2.0


def inverse_elt(N, g):
    return pow(int(g), -1, 2 * N)


def step_elt(o, step):
    """the element of a step of the hoisted calls: step 0 is the identity"""
    return 1 if step == 0 else o.galois_elt(step)


def permuted_key(o, g, key):
    """step 1: [Ltop][2][K][N], residue polynomial (j, k, i) permuted in NTT form by g^-1 under prime i"""
    gi = inverse_elt(o.N, g)
    out = np.empty_like(key)
    for j in range(key.shape[0]):
        for k in range(2):
            for i in range(o.K):
                out[j, k, i] = o.apply_galois_poly(i, gi, 1, key[j, k, i])
    return out


def _native(o, ct, g, key_p, ntt_form):
    L = ct.shape[1]
    start = np.ascontiguousarray(ct).copy()
    start[1] = 0
    u = o.switch_key(np.ascontiguousarray(ct[1]), key_p, start)
    out = np.empty_like(u)
    for k in range(2):
        for i in range(L):
            out[k, i] = o.apply_galois_poly(i, g, ntt_form, u[k, i])
    return out


def _map_polys(f, ct):
    return np.stack([np.stack([f(i, ct[k, i]) for i in range(ct.shape[1])]) for k in range(ct.shape[0])])


def hoisted(o, ct, g, key, ntt_form=None, key_p=None):
    """ct [2][L][N] -> [2][L][N] under element g; key: key_g (or key_p = permuted_key(o, g, key_g), to build it once for many inputs).
    ntt_form None: the context's own form (CKKS NTT, BFV coefficients); a BFV context with ntt_form 1: ntt(ref(intt(ct)))"""
    from oracle import SCHEME_CKKS
    ckks = o.scheme == SCHEME_CKKS
    if ntt_form is None:
        ntt_form = ckks
    if g == 1:
        return np.ascontiguousarray(ct).copy()
    if key_p is None:
        key_p = permuted_key(o, g, key)
    if ckks:
        assert ntt_form, "CKKS ciphertexts are in NTT form"
        return _native(o, ct, g, key_p, 1)
    if not ntt_form:
        return _native(o, ct, g, key_p, 0)
    return _map_polys(o.ntt, _native(o, _map_polys(o.intt, ct), g, key_p, 0))


def hoisted_many(o, cts, elts, keys, ntt_form=None):
    """cts [n][2][L][N], keys {elt: key} -> [len(elts)][n][2][L][N] (element-major, as the device call lays it out)"""
    kp = {g: permuted_key(o, g, keys[g]) for g in set(elts) if g != 1}
    return np.stack([np.stack([hoisted(o, ct, g, None, ntt_form, kp.get(g)) for ct in cts]) for g in elts])


def plain_sum(o, cts, steps, keys, plains):
    """cts [n][2][L][N] NTT form, plains [len(steps)][L][N] NTT form -> [n][2][L][N]: sum_r multiply_plain(hoisted(ct, step r), plains[r])"""
    terms = hoisted_many(o, cts, [step_elt(o, s) for s in steps], keys, 1)
    out = []
    for i in range(len(cts)):
        acc = None
        for r in range(len(steps)):
            t = o.multiply_plain(terms[r, i], plains[r])
            acc = t if acc is None else o.add(acc, t)
        out.append(acc)
    return np.stack(out)
