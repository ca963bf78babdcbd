"""The definition of he355_combine_scalars_rescale, he355_ckks_eval_chebyshev and he355_ckks_eval_mod (include/he355.h), written once on
the oracle's multiply_ntt / relinearize / rescale / mod_switch_drop / add and on tests/ckks_eval_poly_ref.py's combination.  TEST-ONLY.

Direct recursion on values, like its monomial sibling: the device's plan (csrc/poly_args.h with the Chebyshev basis) is a different spelling
of the same definition, and the tests hold the two to each other bit for bit.  All scale arithmetic is Python floats (IEEE doubles) in the
order the header writes it."""
import math

import numpy as np

import ckks_eval_poly_ref as ref


def combine_rescale(ctx, L, terms, scalars, const=None, composed=False):
    """he355_combine_scalars_rescale: the combination at level L into a temporary, then the oracle's rescale: [size][L - 1][N]"""
    c = ref.combine_composed(ctx, L, terms, scalars, const) if composed else ref.combine(ctx.moduli, L, terms, scalars, const)
    return ctx.rescale(c)


def cheb_split(p, e):
    """p = lo + T_e hi in the Chebyshev basis (2e > deg p): hi[0] = c_e; for k = e + 1 .. deg in increasing order hi[k - e] = 2.0 * c_k and
    lo[2e - k] = lo[2e - k] - c_k; lo trimmed"""
    hi, lo = [0.0] * (len(p) - e), list(p[:e])
    hi[0] = p[e]
    for k in range(e + 1, len(p)):
        hi[k - e] = 2.0 * p[k]
        lo[2 * e - k] = lo[2 * e - k] - p[k]
    return hi, ref.trimmed(lo)


class Evaluator(ref.Evaluator):
    """sum_k c_k T_k(u) on one ciphertext [2][L][N] at scale in_scale.  The monomial evaluator's tree with T_k for x^k: the powers end in
    a fused step (2 P - W, or 2 P - (W / s_1) T_1), a leaf is ONE fused step, a node splits in the Chebyshev basis.  counters(): `rescales`
    counts the fused steps."""

    def _split(self, p):
        e = self.giant(len(p) - 1)
        hi, lo = cheb_split(p, e)
        assert all(math.isfinite(v) for v in hi + lo)
        return e, hi, lo

    def _fused(self, L, terms, scalars, const=None):
        self.rescales += 1
        if self.x is None:
            return None
        return self.o.rescale(self._combine(L, terms, scalars, const))

    def _run(self):
        self.products = self.combinations = self.rescales = self.adds = 0
        self.dropped = set()
        self.min_scalar_bits = -1
        self.level, self.scale, self.val = {1: self.L}, {1: self.in_scale}, {1: self.x}
        q = self.q
        for k in self.powers:
            b, a = k // 2, k - k // 2
            l = min(self.level[a], self.level[b])
            W = self.scale[a] * self.scale[b]
            da, db = self._drop(a, l), self._drop(b, l)
            self.products += 1
            P = None if self.x is None else self.o.relinearize(self.o.multiply_ntt(da, db), self.rk)
            two = [2] * l
            if k % 2 == 0:
                self.val[k] = self._fused(l, [P], [two], ref.scalar_residues(q, l, -W))
            else:
                self.val[k] = self._fused(l, [P, self.x], [two, ref.scalar_residues(q, l, -(W / self.scale[1]))])
            self.level[k] = l - 1
            self.scale[k] = W / float(q[l - 1])
        out = self._eval(self.p, self.L_out, self.out_scale)
        self.drops = len(self.dropped)
        return out

    def _leaf(self, terms, const, Lt):
        Lc = Lt + 1
        for k, v in terms:
            assert self.level[k] >= Lc
            a = abs(int(round(v)))
            if a:
                b = a.bit_length() - 1
                self.min_scalar_bits = b if self.min_scalar_bits < 0 else min(self.min_scalar_bits, b)
        return self._fused(Lc, [self.val[k] for k, _ in terms], [ref.scalar_residues(self.q, Lc, v) for _, v in terms],
                           None if const is None else ref.scalar_residues(self.q, Lc, const))


def eval_chebyshev(ctx, x, coeffs, log_baby, in_scale, out_scale, rk, composed=False):
    ev = Evaluator(ctx, coeffs, log_baby, x.shape[1], in_scale, out_scale, rk, composed)
    return ev.run(x), ev


def mod_scales(moduli, l0, r, out_scale):
    """(S_0, [s_0 .. s_r]): S_r = out_scale, S_(j-1) = sqrt(S_j * q[l_j]) backwards; s_0 = S_0, s_j = (s_(j-1) * s_(j-1)) / q[l_j]"""
    S = out_scale
    for j in range(r, 0, -1):
        S = math.sqrt(S * float(moduli[l0 - j]))
    s = [S]
    for j in range(1, r + 1):
        s.append((s[-1] * s[-1]) / float(moduli[l0 - j]))
    return S, s


class ModEvaluator:
    """he355_ckks_eval_mod: the Chebyshev part at the target S_0, then r steps y <- 2 y^2 - 1.  run(x) -> [2][L - depth - r][N];
    counters() as the plan states them (products and combinations include the steps'), out_scale = s_r."""

    def __init__(self, ctx, coeffs, log_baby, L, in_scale, out_scale, r, rk=None, composed=False):
        self.o, self.rk, self.r = ctx, rk, r
        probe = Evaluator(ctx, coeffs, log_baby, L, in_scale, out_scale, rk, composed)
        self.l0 = L - probe.depth
        assert probe.depth + r < L
        self.S0, self.s = mod_scales(ctx.moduli, self.l0, r, out_scale)
        self.ev = Evaluator(ctx, coeffs, log_baby, L, in_scale, self.S0, rk, composed)
        self.depth, self.L_out, self.out_scale = probe.depth + r, self.l0 - r, self.s[-1]

    def _steps(self, y):
        for j in range(1, self.r + 1):
            lj = self.l0 - j
            self.ev.products += 1
            self.ev.combinations += 1
            if y is not None:
                z = self.o.rescale(self.o.relinearize(self.o.multiply_ntt(y, y), self.rk))
                y = self.ev._combine(lj, [z], [[2] * lj], ref.scalar_residues(self.o.moduli, lj, -self.s[j]))
        return y

    def count(self):
        self.ev.count()
        self._steps(None)

    def run(self, x):
        return self._steps(self.ev.run(x))

    def counters(self):
        c = self.ev.counters()
        c.update(depth=self.depth, L_out=self.L_out, double_angles=self.r)
        return c


def eval_mod(ctx, x, coeffs, log_baby, in_scale, out_scale, r, rk, composed=False):
    ev = ModEvaluator(ctx, coeffs, log_baby, x.shape[1], in_scale, out_scale, r, rk, composed)
    return ev.run(x), ev


def eval_mod_coeffs(K, r, degree):
    """the Chebyshev interpolant of cos((2 pi / 2^r) (K u - 1/4)) on [-1, 1] (the binding's eval_mod_coeffs)"""
    w = 2.0 * np.pi / float(1 << r)
    return [float(c) for c in np.polynomial.chebyshev.chebinterpolate(lambda u: np.cos(w * (K * u - 0.25)), degree)]


def double_angles(y, r):
    for _ in range(r):
        y = 2.0 * y * y - 1.0
    return y


def yardstick(ctx, x, coeffs, log_baby, in_scale, out_scale, r, rk):
    """The accuracy yardstick: the MONOMIAL tree (ckks_eval_poly_ref.Evaluator) on cheb2poly of the same coefficients at the same target
    scale, then r double angles through the oracle's public calls.  Returns (ciphertext, its scale)."""
    import oracle as ho
    mono = [float(c) for c in np.polynomial.chebyshev.cheb2poly(np.array(coeffs))]
    probe = ref.Evaluator(ctx, mono, log_baby, x.shape[1], in_scale, out_scale, rk)
    l0 = x.shape[1] - probe.depth
    S0, s = mod_scales(ctx.moduli, l0, r, out_scale)
    y = ref.Evaluator(ctx, mono, log_baby, x.shape[1], in_scale, S0, rk).run(x)
    N = ctx.N
    for j in range(1, r + 1):
        lj = l0 - j
        z = ctx.rescale(ctx.relinearize(ctx.multiply_ntt(y, y), rk))
        y = ctx.add(z, z)
        y = ctx.add_plain(y, ho.ckks_encode(ctx, np.full(N // 2, -1.0), s[j], lj))
    return y, s[-1]
