#!/usr/bin/env python3
"""EvalMod's pieces on one MI355X, n ciphertexts (default 64):
  fused     ONE he355_combine_scalars_rescale against the two calls it equals, he355_combine_scalars into a temporary + he355_rescale, at
            T = 1, 2 and 8 terms (a constant included), with the verdict of tools/probe_common.py (the fused median against the
            composition's median and spread).
  call      ONE he355_ckks_eval_chebyshev against the SAME tree (tests/ckks_eval_mod_ref.py walks it) driven through the public calls --
            he355_multiply_relin, he355_mod_switch_drop, he355_add, and he355_combine_scalars + he355_rescale where the call runs a fused
            step -- for a dense degree 15 and a dense degree 31, log_baby 1.
  evalmod   he355_ckks_eval_mod at (K = 12, r = 3, degree 31), depth 8, where the chain holds it (in_scale = the chain's scale).
The shapes:
  ckks8192    CKKS N = 8192 {60, 40 x 5, 60}   (L = 6)
  ckks16384   CKKS N = 16384 {60, 45 x 5, 60}  (L = 6)
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain)
The candidates alternate inside one process, every one is warmed up first, and the figures are min / median / max over the regions
(tools/probe_common.py).  The relinearization key and the inputs are synthetic (uniform residues): nothing timed depends on what they hold.
Usage: python tools/ckks_eval_mod_probe.py [regions] [calls per region] [all | ckks8192 | ckks16384 | headline] [n]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ckks_eval_mod_ref as mref
from tools.probe_common import alternated, fmt, verdict

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
which = sys.argv[3] if len(sys.argv) > 3 else "all"
n_cts = int(sys.argv[4]) if len(sys.argv) > 4 else 64
SHAPES = {
    "ckks8192": (8192, [60, 40, 40, 40, 40, 40, 60], 2.0 ** 40),
    "ckks16384": (16384, [60, 45, 45, 45, 45, 45, 60], 2.0 ** 45),
    "headline": (32768, be.chain_bits(16, 45), 2.0 ** 45),
}
POLYS = {15: [0.2 - 0.01 * k for k in range(16)], 31: [0.2 - 0.005 * k for k in range(32)]}


class Slab:
    """a device batch [n][2][L][N] as the reference's walk sees a ciphertext: .shape[1] is its level"""

    def __init__(self, buf, L, N):
        self.buf, self.shape = buf, (2, L, N)


class Composed:
    """the oracle's interface on device slabs, for mref.Evaluator: the tree through the public calls"""

    def __init__(self, g, n):
        self.g, self.n, self.N, self.moduli = g, n, g.N, g.moduli
        self.live = []
        self.ix = be.Context.pairwise()

    def new(self, L):
        s = Slab(self.g.alloc(self.n * 2 * L * self.N), L, self.N)
        self.live.append(s.buf)
        return s

    def release(self):
        for b in self.live:
            b.free()
        self.live = []
        self.g._bufs = [b for b in self.g._bufs if b.ptr]

    def multiply_ntt(self, a, b):
        return ("product", a, b)

    def relinearize(self, prod, rk):
        return prod

    def _product(self, v, rescale):
        _, a, b = v
        L = a.shape[1]
        out = self.new(L - 1 if rescale else L)
        self.g.multiply_relin(L, self.n, a.buf, b.buf, self.ix, out.buf, rescale=rescale)
        return out

    def rescale(self, v):
        if isinstance(v, tuple):
            return self._product(v, True)
        L = v.shape[1]
        out = self.new(L - 1)
        self.g.rescale(L, 2, self.n, v.buf, out.buf)
        return out

    def mod_switch_drop(self, v, L_to):
        out = self.new(L_to)
        self.g.mod_switch_drop(v.shape[1], L_to, self.n * 2, v.buf, out.buf)
        return out

    def add(self, a, b):
        out = self.new(a.shape[1])
        self.g.add(a.shape[1], 2, self.n, a.buf, b.buf, self.ix, out.buf)
        return out

    def combine(self, L, terms, scalars, const=None):
        terms = [self._product(t, False) if isinstance(t, tuple) else t for t in terms]  # a power's product, without its rescale
        out = self.new(L)
        self.g.combine_scalars(L, 2, self.n, [(t.buf, t.shape[1]) for t in terms], scalars, out.buf, const)
        return out


def composed_tree(g, n, src, L, coeffs, log_baby, scale):
    o = Composed(g, n)
    ev = mref.Evaluator(o, coeffs, log_baby, L, scale, scale, rk=None)
    ev._combine = o.combine
    x = Slab(src, L, g.N)

    def run():
        ev.x = x
        ev._run()
        o.release()

    return run, ev


def run(name, n):
    N, bits, scale = SHAPES[name]
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False, device=0)
    g.set_relin_key_synthetic(5)
    L = g.L
    per = 2 * L * N
    q = g.moduli
    print(f"== {name}: N = {N} {bits if len(bits) < 10 else '{60, 45 x 15, 60}'}  L = {L}  n = {n}", flush=True)
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls")
    slabs = [g.alloc(n * per) for _ in range(8)]  # eight distinct slabs: every term's bytes come from HBM
    for k, b in enumerate(slabs):
        g.fill_uniform(b, n * 2 * L, list(range(L)), 7 + k)
    src = slabs[0]
    out, tmp = g.alloc(n * per), g.alloc(n * per)
    cst = [q[i] - 1 for i in range(L)]
    for t in (1, 2, 8):
        terms = [(slabs[k], L) for k in range(t)]
        scalars = [[(12345 + 977 * k + i) % q[i] for i in range(L)] for k in range(t)]

        def fused(terms=terms, scalars=scalars):
            g.combine_scalars_rescale(L, 2, n, terms, scalars, out, cst)

        def two(terms=terms, scalars=scalars):
            g.combine_scalars(L, 2, n, terms, scalars, tmp, cst)
            g.rescale(L, 2, n, tmp, out)

        tf, tt = alternated(g, [fused, two], [calls * 4] * 2, repeats)
        spread, word = verdict(tf, tt)
        print(f"   fused  T = {t}: he355_combine_scalars_rescale {fmt(tf)}   combine + rescale {fmt(tt)}   two / fused {tt[1] / tf[1]:5.2f}   "
              f"(spread {spread:.1f}: {word})", flush=True)
    for deg, coeffs in POLYS.items():
        pl = g.ckks_eval_chebyshev_plan(L, coeffs, 1, scale, scale, n)

        def call():
            g.ckks_eval_chebyshev(L, n, src, coeffs, 1, scale, scale, out)

        tree, ev = composed_tree(g, n, src, L, coeffs, 1, scale)
        tc, tt = alternated(g, [call, tree], [calls] * 2, repeats, warmup=1)
        print(f"   call   degree {deg:2d}: depth {pl['depth']}, {pl['products']} products, {pl['rescales']} fused steps, pool bound {pl['pool_bytes'] / 2 ** 20:7.0f} MiB   "
              f"he355_ckks_eval_chebyshev {fmt(tc)}   composed {fmt(tt)}   composed / call {tt[1] / tc[1]:5.2f}", flush=True)
    K, r, deg = 12, 3, 31
    coeffs = be.eval_mod_coeffs(K, r, deg)
    # in_scale = the chain's scale: nothing timed depends on the scales, and q_0 * K against this chain's 45-bit primes lets the powers'
    # scales s_k = s_a s_b / q grow with k until a scalar passes 2^126 (EvalMod's primes are chosen near q_0 * K: include/he355.h)
    try:
        pl = g.ckks_eval_mod_plan(L, coeffs, 1, scale, scale, r, n)
    except be.HE355Error as e:
        print(f"   evalmod ({K}, {r}, {deg}): refused at L = {L}: {e}")
    else:
        t, = alternated(g, [lambda: g.ckks_eval_mod(L, n, src, coeffs, 1, scale, scale, r, out)], [calls], repeats, warmup=1)
        print(f"   evalmod ({K}, {r}, {deg}): depth {pl['depth']} (L_out {pl['L_out']}), {pl['products']} products, {pl['rescales']} fused steps, {pl['combinations']} combinations, "
              f"min_scalar_bits {pl['min_scalar_bits']}   {fmt(t)}", flush=True)
    print(f"   he355_cheb_stats: {g.cheb_stats()}", flush=True)
    g.close()


if __name__ == "__main__":
    for name in SHAPES:
        if which in ("all", name):
            run(name, n_cts)
