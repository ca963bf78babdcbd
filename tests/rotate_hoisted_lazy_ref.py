"""The definition of the lazy-mod-down ("double-hoisted") plain sum (include/he355.h: he355_rotate_hoisted_plain_sum_lazy) and of
he355_plain_extend_special, from Python integers and the oracle's transforms and permutations only.  For a size-2 NTT-form ciphertext
(c0, c1) at level L, steps s_r with elements g_r (step 0: the identity) and plaintexts plain_qp [R][L + 1][N] in NTT form -- rows 0 .. L - 1
under the data primes, row L under the special prime P = q_{K-1}:

  1. digits, once:   d_j = iNTT_j(c1[j]);  d^_{j,i} = c1[j] if i == j else NTT_i(d_j mod q_i), i over the L data primes and P
  2. per keyed r:    key'_r = rotate_hoisted_ref.permuted_key(g_r);  S_r[k][i] = sum_j d^_{j,i} (.) key'_r[j][k][i]      (no mod-down)
  3. in Q P:         A[k][i] = sum_{r keyed} sigma_{g_r}(S_r[k][i]) (.) plain_qp[r][i]
  4. in Q:           B[0][i] = sum_{r keyed} sigma_{g_r}(c0[i]) (.) plain_qp[r][i] + sum_{r identity} c0[i] (.) plain_qp[r][i]
                     B[1][i] = sum_{r identity} c1[i] (.) plain_qp[r][i]
  5. ONE mod-down:   out[k][i] = B[k][i] + (A[k][i] - NTT_i(delta_i)) P^-1 mod q_i,  h = floor(P / 2),  rho = (iNTT_P(A[k][L]) + h) mod P,
                     delta_i = (rho mod q_i - h mod q_i) mod q_i

A sum with no keyed element is B alone.  Not the bits of rotate_hoisted_ref.plain_sum (a sum of mod-downs; this is the mod-down of a sum),
but the same plaintext after decryption.  No GPU, no backend."""
import numpy as np

import rotate_hoisted_ref as eager


def _obj(a):
    return np.asarray(a).astype(object)


def _u64(a):
    return np.asarray(a, dtype=object).astype(np.uint64)


def mulmod(a, b, q):
    return _u64((_obj(a) * _obj(b)) % q)


def addmod(a, b, q):
    return _u64((_obj(a) + _obj(b)) % q)


def key_primes(o, L):
    """the primes of a level-L key product: the L data primes and the special prime (indices into the key chain)"""
    return list(range(L)) + [o.K - 1]


def digits(o, c1):
    """step 1: [L][L + 1][N], digit j under prime key_primes[idx]"""
    L = c1.shape[0]
    out = np.empty((L, L + 1, o.N), dtype=np.uint64)
    for j in range(L):
        d = o.intt(j, c1[j])
        for idx, i in enumerate(key_primes(o, L)):
            out[j, idx] = c1[j] if i == j else o.ntt(i, d % np.uint64(o.moduli[i]))
    return out


def key_product(o, dig, key_p):
    """step 2: [2][L + 1][N], canonical NTT form, no mod-down"""
    L = dig.shape[0]
    out = np.empty((2, L + 1, o.N), dtype=np.uint64)
    for k in range(2):
        for idx, i in enumerate(key_primes(o, L)):
            acc = np.zeros(o.N, dtype=object)
            for j in range(L):
                acc = acc + _obj(dig[j, idx]) * _obj(key_p[j, k, i])
            out[k, idx] = _u64(acc % o.moduli[i])
    return out


def mod_down(o, A, B):
    """step 5: A [2][L + 1][N], B [2][L][N] -> [2][L][N]"""
    L = B.shape[1]
    sp = o.K - 1
    P = o.moduli[sp]
    h = P // 2
    out = np.empty_like(B)
    for k in range(2):
        rho = (_obj(o.intt(sp, A[k, L])) + h) % P
        for i in range(L):
            q = o.moduli[i]
            delta = o.ntt(i, _u64((rho % q - h % q) % q))
            x = ((_obj(A[k, i]) - _obj(delta)) * pow(P, -1, q) + _obj(B[k, i])) % q
            out[k, i] = _u64(x)
    return out


def plain_sum_lazy(o, cts, steps, keys, plain_qp):
    """cts [n][2][L][N] NTT form, plain_qp [len(steps)][L + 1][N], keys {elt: key} -> [n][2][L][N]"""
    cts = np.asarray(cts)
    n, _, L, N = cts.shape
    elts = [eager.step_elt(o, s) for s in steps]
    kp = {g: eager.permuted_key(o, g, keys[g]) for g in set(elts) if g != 1}
    primes = key_primes(o, L)
    out = []
    for ct in cts:
        dig = digits(o, ct[1]) if kp else None
        prod = {}
        A = np.zeros((2, L + 1, N), dtype=np.uint64)
        B = np.zeros((2, L, N), dtype=np.uint64)
        for r, g in enumerate(elts):
            if g == 1:
                for k in range(2):
                    for i in range(L):
                        B[k, i] = addmod(B[k, i], mulmod(ct[k, i], plain_qp[r, i], o.moduli[i]), o.moduli[i])
                continue
            if g not in prod:
                prod[g] = key_product(o, dig, kp[g])
            S = prod[g]
            for k in range(2):
                for idx, i in enumerate(primes):
                    q = o.moduli[i]
                    A[k, idx] = addmod(A[k, idx], mulmod(o.apply_galois_poly(i, g, 1, S[k, idx]), plain_qp[r, idx], q), q)
            for i in range(L):
                q = o.moduli[i]
                B[0, i] = addmod(B[0, i], mulmod(o.apply_galois_poly(i, g, 1, ct[0, i]), plain_qp[r, i], q), q)
        out.append(mod_down(o, A, B) if kp else B)
    return np.stack(out)


def extend_special(o, plain_ntt):
    """plain_ntt [L][N] NTT form -> ([L + 1][N], mismatches): rows copied; row L = NTT_P(c mod P), c the coefficients under prime 0 centred
    into (-q_0 / 2, q_0 / 2]; mismatches = the (coefficient, prime i >= 1) pairs whose residue is not c mod q_i"""
    plain_ntt = np.asarray(plain_ntt)
    L = plain_ntt.shape[0]
    q0 = o.moduli[0]
    c = _obj(o.intt(0, plain_ntt[0]))
    c = np.where(c > q0 // 2, c - q0, c)
    out = np.empty((L + 1, o.N), dtype=np.uint64)
    out[:L] = plain_ntt
    out[L] = o.ntt(o.K - 1, _u64(c % o.moduli[o.K - 1]))
    bad = 0
    for i in range(1, L):
        bad += int((_obj(o.intt(i, plain_ntt[i])) != c % o.moduli[i]).sum())
    return out, bad


def ones_qp(o, L):
    """the NTT form of the constant 1 on all L + 1 rows"""
    return np.ones((L + 1, o.N), dtype=np.uint64)
