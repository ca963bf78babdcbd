"""The definition of he355_combine_scalars, he355_ckks_scalar_residues and he355_ckks_eval_poly (include/he355.h), written once on the
oracle's multiply_ntt / relinearize / rescale / mod_switch_drop / add and Python integers.  TEST-ONLY.

Everything here is direct recursion on values: no step list, no buffers -- the device's plan (csrc/poly_args.h) is a different spelling of
the same definition, and the tests hold the two to each other bit for bit.  All scale arithmetic is Python floats (IEEE doubles) in the
order the header writes it."""
import numpy as np


def scalar_residues(moduli, L, v):
    """the residues of the integer nearest v (ties to even: Python's round) under the first L primes"""
    a = int(round(v))
    return [a % q for q in moduli[:L]]


def combine(moduli, L, terms, scalars, const=None):
    """terms: arrays [size][L_t][N], L_t >= L (rows >= L ignored); scalars: per term L residues; const: L residues, added to
    polynomial 0.  The integer sum, reduced once."""
    size, _, N = terms[0].shape
    out = np.empty((size, L, N), dtype=np.uint64)
    for k in range(size):
        for i in range(L):
            q = moduli[i]
            acc = np.zeros(N, dtype=object)
            for t, a in zip(terms, scalars):
                acc = acc + t[k, i].astype(object) * int(a[i])
            if const is not None and k == 0:
                acc = acc + int(const[i])
            out[k, i] = np.array([int(x) % q for x in acc], dtype=np.uint64)
    return out


def combine_composed(ctx, L, terms, scalars, const=None):
    """The same combination composed from the oracle's own calls -- mod_switch_drop, multiply_plain by the all-a NTT vector, add, add_plain
    of the all-c vector: tests/test_ckks_eval_poly_ref_cpu.py holds it equal to combine() bit for bit, and the large GPU cases use it."""
    N = ctx.N
    flat = lambda a: np.repeat(np.array([int(v) for v in a[:L]], dtype=np.uint64)[:, None], N, axis=1)
    acc = None
    for t, a in zip(terms, scalars):
        td = t if t.shape[1] == L else ctx.mod_switch_drop(t, L)
        prod = ctx.multiply_plain(td, flat(a))
        acc = prod if acc is None else ctx.add(acc, prod)
    return acc if const is None else ctx.add_plain(acc, flat(const))


def clog2(k):
    return (k - 1).bit_length()


def trimmed(c):
    c = [float(x) for x in c]
    while c and c[-1] == 0.0:
        c.pop()
    return c


class Evaluator:
    """p(x) on one ciphertext x [2][L][N] at scale in_scale.  run(): the result [2][L - depth][N]; afterwards the counters say what the
    definition used: products, combinations, rescales, drops, adds, powers, min_scalar_bits."""

    def __init__(self, ctx, coeffs, log_baby, L, in_scale, out_scale, rk=None, composed=False):
        self.o, self.q, self.rk = ctx, ctx.moduli, rk
        # composed: combinations through combine_composed (the oracle's own calls; the same bits, faster on large rings)
        self._combine = (lambda L, t, s, c=None: combine_composed(ctx, L, t, s, c)) if composed else (lambda L, t, s, c=None: combine(ctx.moduli, L, t, s, c))
        self.p, self.m, self.L = trimmed(coeffs), 1 << log_baby, L
        self.in_scale, self.out_scale = in_scale, out_scale
        assert len(self.p) >= 2
        self.depth = self._depth(self.p)
        assert self.depth < L
        self.L_out = L - self.depth
        self.degree = len(self.p) - 1
        # the powers the leaves and the splits use, closed under the halves
        need = set()
        self._mark(self.p, need)
        for k in sorted(need, reverse=True):
            self._halves(k, need)
        self.powers = sorted(k for k in need if k >= 2)

    def _halves(self, k, need):
        if k >= 2:
            for h in (k // 2, k - k // 2):
                if h not in need:
                    need.add(h)
                    self._halves(h, need)

    def giant(self, deg):
        e = self.m
        while 2 * e <= deg:
            e *= 2
        return e

    def _split(self, p):
        e = self.giant(len(p) - 1)
        return e, p[e:], trimmed(p[:e])

    def _depth(self, p):
        deg = len(p) - 1
        if deg < self.m:
            return 1 + max(clog2(k) for k in range(1, deg + 1) if p[k] != 0.0)
        e, hi, lo = self._split(p)
        dh = 1 + clog2(e) if len(hi) == 1 else 1 + max(self._depth(hi), clog2(e))
        return max(dh, self._depth(lo)) if len(lo) >= 2 else dh

    def _mark(self, p, need):
        deg = len(p) - 1
        if deg < self.m:
            need.update(k for k in range(1, deg + 1) if p[k] != 0.0)
            return
        e, hi, lo = self._split(p)
        need.add(e)
        if len(hi) >= 2:
            self._mark(hi, need)
        if len(lo) >= 2:
            self._mark(lo, need)

    # ---- the counters alone (no ciphertext): what a brute-force walk of the definition uses
    def count(self):
        self.x = None
        return self._run()

    def run(self, x):
        self.x = np.ascontiguousarray(x)
        return self._run()

    def _run(self):
        self.products = self.combinations = self.rescales = self.adds = 0
        self.dropped = set()
        self.min_scalar_bits = -1
        self.level, self.scale, self.val = {1: self.L}, {1: self.in_scale}, {1: self.x}
        for k in self.powers:
            f, c = k // 2, k - k // 2
            l = min(self.level[f], self.level[c])
            self.level[k] = l - 1
            self.scale[k] = self.scale[f] * self.scale[c] / float(self.q[l - 1])
            self.val[k] = self._mulr(self._drop(f, l), self._drop(c, l))
        out = self._eval(self.p, self.L_out, self.out_scale)
        self.drops = len(self.dropped)
        return out

    def _mulr(self, a, b):
        self.products += 1
        if a is None:
            return None
        return self.o.rescale(self.o.relinearize(self.o.multiply_ntt(a, b), self.rk))

    def _drop(self, k, l):
        assert self.level[k] >= l
        if self.level[k] > l:
            self.dropped.add((k, l))
        v = self.val[k]
        return None if v is None else (v if self.level[k] == l else self.o.mod_switch_drop(v, l))

    def _leaf(self, terms, const, Lt):
        """terms: (exponent, scalar as a float); const: a float or None; one combination at Lt + 1, then the rescale"""
        Lc = Lt + 1
        for k, v in terms:
            assert self.level[k] >= Lc
            a = abs(int(round(v)))
            if a:
                b = a.bit_length() - 1
                self.min_scalar_bits = b if self.min_scalar_bits < 0 else min(self.min_scalar_bits, b)
        self.combinations += 1
        self.rescales += 1
        if self.x is None:
            return None
        c = self._combine(Lc, [self.val[k] for k, _ in terms], [scalar_residues(self.q, Lc, v) for _, v in terms],
                    None if const is None else scalar_residues(self.q, Lc, const))
        return self.o.rescale(c)

    def _eval(self, p, Lt, S):
        deg = len(p) - 1
        T = S * float(self.q[Lt])
        if deg < self.m:
            return self._leaf([(k, (p[k] * T) / self.scale[k]) for k in range(1, deg + 1) if p[k] != 0.0], p[0] * T if p[0] != 0.0 else None, Lt)
        e, hi, lo = self._split(p)
        if len(hi) == 1:
            prod = self._leaf([(e, (hi[0] * T) / self.scale[e])], None, Lt)
        else:
            H = self._eval(hi, Lt + 1, T / self.scale[e])
            prod = self._mulr(H, self._drop(e, Lt + 1))
        if not lo:
            return prod
        if len(lo) == 1:
            self.combinations += 1
            if self.x is None:
                return None
            return self._combine(Lt, [prod], [[1] * Lt], scalar_residues(self.q, Lt, lo[0] * S))
        LO = self._eval(lo, Lt, S)
        self.adds += 1
        return None if self.x is None else self.o.add(prod, LO)

    def counters(self):
        return {"depth": self.depth, "L_out": self.L_out, "degree": self.degree, "products": self.products, "combinations": self.combinations,
                "rescales": self.rescales, "drops": self.drops, "adds": self.adds, "powers": len(self.powers), "min_scalar_bits": self.min_scalar_bits}


def eval_poly(ctx, x, coeffs, log_baby, in_scale, out_scale, rk, composed=False):
    ev = Evaluator(ctx, coeffs, log_baby, x.shape[1], in_scale, out_scale, rk, composed)
    return ev.run(x), ev


def horner(ctx, x, coeffs, scale, rk):
    """The reference route of the accuracy bound: Horner with the oracle's multiply_plain / add_plain / multiply_ntt / rescale and full
    constant plaintexts, one level per degree.  Returns (ciphertext, its scale)."""
    import oracle as ho
    c = trimmed(coeffs)
    N = ctx.N
    const = lambda v, s, L: ho.ckks_encode(ctx, np.full(N // 2, v), s, L)
    L = x.shape[1]
    acc = ctx.rescale(ctx.multiply_plain(x, const(c[-1], scale, L)))  # c_d x
    s = scale * scale / float(ctx.moduli[L - 1])
    L -= 1
    for k in range(len(c) - 2, -1, -1):
        if c[k] != 0.0:
            acc = ctx.add_plain(acc, const(c[k], s, L))
        if k == 0:
            break
        xk = ctx.mod_switch_drop(x, L)
        acc = ctx.rescale(ctx.relinearize(ctx.multiply_ntt(acc, xk), rk))
        s = s * scale / float(ctx.moduli[L - 1])
        L -= 1
    return acc, s
