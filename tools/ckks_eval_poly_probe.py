#!/usr/bin/env python3
"""CKKS polynomial evaluation on one MI355X, n = 64 ciphertexts:
  call      ONE he355_ckks_eval_poly against the SAME tree (tests/ckks_eval_poly_ref.py walks it) driven through the public calls with
            constant plaintexts: he355_multiply_relin for the products, and per leaf he355_mod_switch_drop + he355_multiply_plain +
            he355_add per term, he355_add_plain, he355_rescale -- for a dense degree 7 and a dense degree 15, log_baby 1.  The constant
            plaintexts ([L][N] slabs of one residue each) are made once, outside the timed regions.
  rate      k_scalar_combine over 2, 4 and 8 terms (he355_combine_scalars, a constant included) beside k_addsub (he355_add of two slabs) in
            the same run, in bytes moved: T + 1 slabs against 3.
  trade     log_baby 1 against 2: levels used, products, microseconds.
The shapes are the rings of the hoisted probes with chains long enough for degree 15 at log_baby 2 (depth 5):
  ckks8192    CKKS N = 8192 {60, 40 x 5, 60}   (L = 6)
  ckks16384   CKKS N = 16384 {60, 45 x 5, 60}  (L = 6)
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain)
The candidates alternate inside one process, every one is warmed up first, and the figures are min / median / max over the regions
(tools/probe_common.py).  The relinearization key and the inputs are synthetic (uniform residues): nothing timed depends on what they hold.
Usage: python tools/ckks_eval_poly_probe.py [regions] [calls per region] [all | ckks8192 | ckks16384 | headline]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import ckks_eval_poly_ref as ref
from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
which = sys.argv[3] if len(sys.argv) > 3 else "all"
SHAPES = {
    "ckks8192": (8192, [60, 40, 40, 40, 40, 40, 60], 2.0 ** 40),
    "ckks16384": (16384, [60, 45, 45, 45, 45, 45, 60], 2.0 ** 45),
    "headline": (32768, be.chain_bits(16, 45), 2.0 ** 45),
}
POLYS = {7: [0.3 + 0.01 * k for k in range(8)], 15: [0.2 - 0.01 * k for k in range(16)]}


class Slab:
    """a device batch [n][2][L][N] as the reference's walk sees a ciphertext: .shape[1] is its level"""

    def __init__(self, buf, L, N):
        self.buf, self.shape = buf, (2, L, N)


class Composed:
    """the oracle's interface on device slabs, for ref.Evaluator: the tree through the public calls with constant plaintexts"""

    def __init__(self, g, n):
        self.g, self.n, self.N, self.moduli = g, n, g.N, g.moduli
        self.consts, self.live = {}, []
        self.ix = be.Context.pairwise()
        self.one = be.Context.outer(0, n, 0, 1)  # ciphertext r, the one plaintext

    def new(self, L):
        s = Slab(self.g.alloc(self.n * 2 * L * self.N), L, self.N)
        self.live.append(s.buf)
        return s

    def release(self):
        for b in self.live:
            b.free()
        self.live = []
        self.g._bufs = [b for b in self.g._bufs if b.ptr]

    def const(self, L, residues):
        key = (L, tuple(int(v) for v in residues))
        if key not in self.consts:
            self.consts[key] = self.g.to_device(np.repeat(np.array(key[1], dtype=np.uint64)[:, None], self.N, axis=1))
        return self.consts[key]

    def multiply_ntt(self, a, b):
        return ("product", a, b)

    def relinearize(self, prod, rk):
        return prod

    def rescale(self, v):
        if isinstance(v, tuple):
            _, a, b = v
            L = a.shape[1]
            out = self.new(L - 1)
            self.g.multiply_relin(L, self.n, a.buf, b.buf, self.ix, out.buf, rescale=True)
            return out
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
        acc, tmp = self.new(L), self.new(L)
        for k, (t, a) in enumerate(zip(terms, scalars)):
            td = t if t.shape[1] == L else self.mod_switch_drop(t, L)
            self.g.multiply_plain(L, 2, self.n, td.buf, self.const(L, a), self.one, (acc if k == 0 else tmp).buf)
            if k:
                self.g.add(L, 2, self.n, acc.buf, tmp.buf, self.ix, acc.buf)
        if const is not None:
            self.g.add_plain(L, 2, self.n, acc.buf, self.const(L, const), self.one, acc.buf)
        return acc


def composed_tree(g, n, src, L, coeffs, log_baby, scale):
    o = Composed(g, n)
    ev = ref.Evaluator(o, coeffs, log_baby, L, scale, scale, rk=None)
    ev._combine = o.combine
    x = Slab(src, L, g.N)

    def run():
        ev.x = x
        ev._run()
        o.release()

    return run, ev


def run(name, n=64):
    N, bits, scale = SHAPES[name]
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False, device=0)
    g.set_relin_key_synthetic(5)
    L = g.L
    per = 2 * L * N
    print(f"== {name}: N = {N} {bits if len(bits) < 10 else '{60, 45 x 15, 60}'}  L = {L}  n = {n}", flush=True)
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls")
    src, other, out = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    g.fill_uniform(src, n * 2 * L, list(range(L)), 7)
    g.fill_uniform(other, n * 2 * L, list(range(L)), 8)
    for deg, coeffs in POLYS.items():
        pl = g.ckks_eval_poly_plan(L, coeffs, 1, scale, scale, n)

        def call():
            g.ckks_eval_poly(L, n, src, coeffs, 1, scale, scale, out)

        tree, ev = composed_tree(g, n, src, L, coeffs, 1, scale)
        tc, tt = alternated(g, [call, tree], [calls] * 2, repeats, warmup=1)
        print(f"   call   degree {deg:2d}: depth {pl['depth']}, {pl['products']} products, {pl['combinations']} combinations, pool bound {pl['pool_bytes'] / 2 ** 20:7.0f} MiB   "
              f"he355_ckks_eval_poly {fmt(tc)}   composed {fmt(tt)}   composed / call {tt[1] / tc[1]:5.2f}", flush=True)
        for lb in (1, 2):
            p = g.ckks_eval_poly_plan(L, coeffs, lb, scale, scale, n)
            t, = alternated(g, [lambda lb=lb: g.ckks_eval_poly(L, n, src, coeffs, lb, scale, scale, out)], [calls], repeats, warmup=1)
            print(f"   trade  degree {deg:2d} log_baby {lb}: depth {p['depth']} (L_out {p['L_out']}), {p['products']} products, {p['combinations']} combinations, "
                  f"min_scalar_bits {p['min_scalar_bits']}   {fmt(t)}", flush=True)
    q = g.moduli
    slabs = [src, other] + [g.alloc(n * per) for _ in range(6)]  # eight distinct slabs: every term's bytes come from HBM
    for k, b in enumerate(slabs[2:]):
        g.fill_uniform(b, n * 2 * L, list(range(L)), 20 + k)

    def add():
        g.add(L, 2, n, src, other, be.Context.pairwise(), out)

    fs, T = [add], (2, 4, 8)
    for t in T:
        terms = [(slabs[k], L) for k in range(t)]
        scalars = [[(12345 + 977 * k + i) % q[i] for i in range(L)] for k in range(t)]
        cst = [q[i] - 1 for i in range(L)]
        fs.append(lambda terms=terms, scalars=scalars, cst=cst: g.combine_scalars(L, 2, n, terms, scalars, out, cst))
    ts = alternated(g, fs, [calls * 4] * len(fs), repeats)
    print(f"   rate   k_addsub {fmt(ts[0])} us = {3 * n * per * 8 / ts[0][1] / 1e6:6.2f} TB/s", flush=True)
    for t, tm in zip(T, ts[1:]):
        print(f"   rate   k_scalar_combine {t} terms {fmt(tm)} us = {(t + 1) * n * per * 8 / tm[1] / 1e6:6.2f} TB/s of {t + 1} slabs", flush=True)
    st = g.poly_stats()
    print(f"   he355_poly_stats: {st}", flush=True)
    g.close()


if __name__ == "__main__":
    for name in SHAPES:
        if which in ("all", name):
            run(name)
