"""The definitions of the complex-slot calls (include/he355.h: he355_ckks_complex_unit, he355_ckks_complex_scalar_residues,
he355_combine_scalars_complex, he355_ckks_eval_poly_complex), written once on the oracle and Python integers.  TEST-ONLY.

J(X) = X^(N/4) + X^(3N/4) decodes to sqrt(2) i in every slot; in NTT form it is u_i where bit (log2 N - 2) of the index is 0 and q_i - u_i
where it is 1, u_i = ctx.ntt(i, J)[0].  A complex scalar at weight W is A + B J with A = round(Re W), B = round(Im W / sqrt 2): the pair
of residues A +- B u_i.  The evaluator is ckks_eval_poly_ref.Evaluator with complex coefficients: the same tree, every scalar a pair."""
import math

import numpy as np

import ckks_eval_poly_ref as real


def j_poly(N):
    """the coefficients of J"""
    j = np.zeros(N, dtype=np.uint64)
    j[N // 4] = j[3 * N // 4] = 1
    return j


def half_of(N):
    """s(e) for every NTT index e: bit (log2 N - 2)"""
    return (np.arange(N) >> (N.bit_length() - 3)) & 1


def units(ctx, L):
    return [int(ctx.ntt(i, j_poly(ctx.N))[0]) for i in range(L)]


def scalar_integers(v_re, v_im):
    return int(round(v_re)), int(round(v_im / math.sqrt(2.0)))


def scalar_residues(moduli, u, L, v_re, v_im):
    """[[(A + B u_i) % q_i], [(A - B u_i) % q_i]]"""
    a, b = scalar_integers(v_re, v_im)
    return [[(a + b * u[i]) % moduli[i] for i in range(L)], [(a - b * u[i]) % moduli[i] for i in range(L)]]


def scalar_plain(ctx, L, v_re, v_im):
    """NTT(A + B J) under the first L primes: the full plaintext the pair stands for, through the oracle's own transform"""
    a, b = scalar_integers(v_re, v_im)
    N = ctx.N
    rows = []
    for i in range(L):
        q = ctx.moduli[i]
        c = np.zeros(N, dtype=np.uint64)
        c[0] = a % q
        c[N // 4] = c[3 * N // 4] = b % q
        rows.append(ctx.ntt(i, c))
    return np.stack(rows)


def picked(s, pair_i):
    """the Python integers pair_i[s(e)] per NTT index, as an object array (the integers may pass 64 bits)"""
    out = np.empty(len(s), dtype=object)
    out[s == 0], out[s == 1] = int(pair_i[0]), int(pair_i[1])
    return out


def combine(moduli, L, terms, scalars, const=None):
    """terms: arrays [size][L_t][N], L_t >= L; scalars: per term a pair of L residues; const: such a pair, added to polynomial 0.  The
    integer sum with the residue picked by s(e), reduced once."""
    size, _, N = terms[0].shape
    s = half_of(N)
    out = np.empty((size, L, N), dtype=np.uint64)
    for k in range(size):
        for i in range(L):
            q = moduli[i]
            acc = np.zeros(N, dtype=object)
            for t, a in zip(terms, scalars):
                acc = acc + t[k, i].astype(object) * picked(s, (a[0][i], a[1][i]))
            if const is not None and k == 0:
                acc = acc + picked(s, (const[0][i], const[1][i]))
            out[k, i] = np.array([int(x) % q for x in acc], dtype=np.uint64)
    return out


def spread(pair, L, N):
    """the pair as a full NTT-form plaintext [L][N]"""
    s = half_of(N)
    return np.stack([np.where(s == 0, np.uint64(pair[0][i]), np.uint64(pair[1][i])) for i in range(L)]).astype(np.uint64)


def combine_composed(ctx, L, terms, scalars, const=None):
    """The same combination from the oracle's own calls: mod_switch_drop, multiply_plain by the spread pair, add, add_plain."""
    N = ctx.N
    acc = None
    for t, a in zip(terms, scalars):
        td = t if t.shape[1] == L else ctx.mod_switch_drop(t, L)
        prod = ctx.multiply_plain(td, spread(a, L, N))
        acc = prod if acc is None else ctx.add(acc, prod)
    return acc if const is None else ctx.add_plain(acc, spread(const, L, N))


def trimmed(c):
    c = [complex(x) for x in c]
    while c and c[-1] == 0:
        c.pop()
    return c


class Evaluator(real.Evaluator):
    """ckks_eval_poly_ref.Evaluator on complex coefficients.  The tree (depth, marks, splits) reads only whether a coefficient is zero, so
    it is the parent's; the leaves and the constant combinations take pairs."""

    def __init__(self, ctx, coeffs, log_baby, L, in_scale, out_scale, rk=None, composed=False):
        p = trimmed(coeffs)
        # the parent's constructor walks zero / non-zero alone: give it markers, then put the complex list in place
        super().__init__(ctx, [1.0 if c != 0 else 0.0 for c in p], log_baby, L, in_scale, out_scale, rk, composed)
        self.p = p
        self.u = units(ctx, L)
        self._ccombine = (lambda L, t, s, c=None: combine_composed(ctx, L, t, s, c)) if composed else (lambda L, t, s, c=None: combine(ctx.moduli, L, t, s, c))

    def _split(self, p):
        e = self.giant(len(p) - 1)
        lo = list(p[:e])
        while lo and lo[-1] == 0:
            lo.pop()
        return e, p[e:], lo

    def _pair(self, L, v):
        return scalar_residues(self.q, self.u, L, v[0], v[1])

    def _leaf(self, terms, const, Lt):
        """terms: (exponent, (re, im) as floats); const: such a pair or None"""
        Lc = Lt + 1
        for k, v in terms:
            assert self.level[k] >= Lc
            for a in scalar_integers(*v):
                if a:
                    b = abs(a).bit_length() - 1
                    self.min_scalar_bits = b if self.min_scalar_bits < 0 else min(self.min_scalar_bits, b)
        self.combinations += 1
        self.rescales += 1
        if self.x is None:
            return None
        c = self._ccombine(Lc, [self.val[k] for k, _ in terms], [self._pair(Lc, v) for _, v in terms], None if const is None else self._pair(Lc, const))
        return self.o.rescale(c)

    def _eval(self, p, Lt, S):
        deg = len(p) - 1
        T = S * float(self.q[Lt])
        part = lambda c, w, s=None: ((c.real * w) / s, (c.imag * w) / s) if s is not None else (c.real * w, c.imag * w)
        if deg < self.m:
            return self._leaf([(k, part(p[k], T, self.scale[k])) for k in range(1, deg + 1) if p[k] != 0], part(p[0], T) if p[0] != 0 else None, Lt)
        e, hi, lo = self._split(p)
        if len(hi) == 1:
            prod = self._leaf([(e, part(hi[0], T, self.scale[e]))], None, Lt)
        else:
            H = self._eval(hi, Lt + 1, T / self.scale[e])
            prod = self._mulr(H, self._drop(e, Lt + 1))
        if not lo:
            return prod
        if len(lo) == 1:
            self.combinations += 1
            if self.x is None:
                return None
            return self._ccombine(Lt, [prod], [[[1] * Lt, [1] * Lt]], self._pair(Lt, part(lo[0], S)))
        LO = self._eval(lo, Lt, S)
        self.adds += 1
        return None if self.x is None else self.o.add(prod, LO)


def eval_poly(ctx, x, coeffs, log_baby, in_scale, out_scale, rk, composed=False):
    ev = Evaluator(ctx, coeffs, log_baby, x.shape[1], in_scale, out_scale, rk, composed)
    return ev.run(x), ev
