"""The definition of the baby-step/giant-step linear transform (include/he355.h: he355_linear_transform_bsgs), from Python integers and the
oracle's transforms and permutations only, on the parts of tests/rotate_hoisted_lazy_ref.py (digits, key_product, mod_down) and
rotate_hoisted_ref.permuted_key.  For a size-2 NTT-form ciphertext (c0, c1) at level L, baby steps b_i, giant steps G_j (step 0: the
identity), plaintexts plain_qp [n_giant][n_baby][L + 1][N] -- pre-rotated by the caller, plain[j][i] = rot_{-G_j}(diag_{G_j + b_i}) -- and an
optional mask [n_giant][n_baby] (zero: the term is absent); all residues canonical, tile idx under prime key_primes[idx] (hoist_qp_prime):

  1. baby terms:  keyed i, element g:  T_i[k][idx] = sigma_g(S_i[k][idx]), S_i the key product of the digits of c1 under key'_g (no mod-down),
                                        and T_i[0][idx] += P sigma_g(c0[idx]) on the data primes
                  identity:             T_i = (P c0, P c1) on the data primes, 0 under P
  2. inner sum:   E_j[k][idx] = sum_{i used} T_i[k][idx] (.) plain[j][i][idx]                      (per used row j; L + 1 primes)
  3. giant step:  identity row: Acc += E_j in Q P.  Keyed row, element h: e_j = mod_down(E_j); S'_j = the key product of the digits of e_j[1]
                  under key'_h; Acc[k] += sigma_h(S'_j[k]), Acc[0] += P sigma_h(e_j[0]) on the data primes
  4. out = mod_down(Acc)

Only USED steps (named by a term that is not masked) need a key.  No GPU, no backend."""
import numpy as np

import rotate_hoisted_lazy_ref as lazy
import rotate_hoisted_ref as eager
from rotate_hoisted_lazy_ref import _obj, _u64, addmod, mulmod


def _sigma_qp(o, g, X, L):
    """sigma_g on every tile of X [2][L + 1][N]"""
    return np.stack([np.stack([o.apply_galois_poly(i, g, 1, X[k, idx]) for idx, i in enumerate(lazy.key_primes(o, L))]) for k in range(2)])


def _p_times(o, c, L):
    """[L][N] -> P c under the data primes"""
    P = o.moduli[o.K - 1]
    return np.stack([_u64((_obj(c[i]) * P) % o.moduli[i]) for i in range(L)])


def keyed_term(o, dig, key_p, g, c0, L):
    """sigma_g(key product) with P sigma_g(c0) folded into polynomial 0 under the data primes: [2][L + 1][N]"""
    T = _sigma_qp(o, g, lazy.key_product(o, dig, key_p), L)
    pc = _p_times(o, np.stack([o.apply_galois_poly(i, g, 1, c0[i]) for i in range(L)]), L)
    for i in range(L):
        T[0, i] = addmod(T[0, i], pc[i], o.moduli[i])
    return T


def used(mask, n_giant, n_baby):
    m = np.ones((n_giant, n_baby), dtype=bool) if mask is None else np.asarray(mask).astype(bool).reshape(n_giant, n_baby)
    return m


def linear_transform_bsgs(o, cts, baby, giant, keys, plain_qp, mask=None):
    """cts [n][2][L][N] NTT form, plain_qp [len(giant)][len(baby)][L + 1][N], keys {elt: key} -> [n][2][L][N]"""
    cts = np.asarray(cts)
    n, _, L, N = cts.shape
    m = used(mask, len(giant), len(baby))
    assert m.any(), "the mask sets no term"
    b_elts, g_elts = [eager.step_elt(o, s) for s in baby], [eager.step_elt(o, s) for s in giant]
    need = {b_elts[i] for i in range(len(baby)) if m[:, i].any()} | {g_elts[j] for j in range(len(giant)) if m[j].any()}
    kp = {g: eager.permuted_key(o, g, keys[g]) for g in need if g != 1}
    primes = lazy.key_primes(o, L)
    zero_q = np.zeros((2, L, N), dtype=np.uint64)
    out = []
    for ct in cts:
        T = {}
        dig = lazy.digits(o, ct[1]) if any(b_elts[i] != 1 and m[:, i].any() for i in range(len(baby))) else None
        for i, g in enumerate(b_elts):
            if not m[:, i].any():
                continue
            if g == 1:
                T[i] = np.zeros((2, L + 1, N), dtype=np.uint64)
                for k in range(2):
                    T[i][k, :L] = _p_times(o, ct[k], L)
            else:
                T[i] = keyed_term(o, dig, kp[g], g, ct[0], L)
        acc = np.zeros((2, L + 1, N), dtype=np.uint64)
        for j, h in enumerate(g_elts):
            if not m[j].any():
                continue
            E = np.zeros((2, L + 1, N), dtype=np.uint64)
            for k in range(2):
                for idx, pi in enumerate(primes):
                    q = o.moduli[pi]
                    s = np.zeros(N, dtype=object)
                    for i in range(len(baby)):
                        if m[j, i]:
                            s = s + _obj(T[i][k, idx]) * _obj(plain_qp[j, i, idx])
                    E[k, idx] = _u64(s % q)
            if h != 1:
                e = lazy.mod_down(o, E, zero_q)
                E = keyed_term(o, lazy.digits(o, e[1]), kp[h], h, e[0], L)
            for k in range(2):
                for idx, pi in enumerate(primes):
                    acc[k, idx] = addmod(acc[k, idx], E[k, idx], o.moduli[pi])
        out.append(lazy.mod_down(o, acc, zero_q))
    return np.stack(out)


def split_diagonals(diags, baby, giant, rot):
    """the pre-rotated operands of a cyclic matrix given by its diagonals: [len(giant)][len(baby)] vectors, entry [j][i] =
    rot(diags[giant[j] + baby[i]], -giant[j]); rot(v, s) rotates a slot vector left by s"""
    return [[rot(diags[G + b], -G) for b in baby] for G in giant]
