#!/usr/bin/env python3
"""Complex CKKS slots on one MI355X, n = 64 ciphertexts:
  rate      k_scalar_combine_cplx over 2, 4 and 8 terms (he355_combine_scalars_complex, a constant pair included) beside k_scalar_combine
            over the same terms and k_addsub (he355_add of two slabs) in the same run, in bytes moved: T + 1 slabs against 3; the ratio of
            the two combinations' medians.
  call      ONE he355_ckks_eval_poly_complex of a dense complex degree 7 (log_baby 1) against the SAME tree (tests/ckks_complex_ref.py
            walks it) through the public calls with complex plaintexts: he355_multiply_relin for the products, and per leaf
            he355_mod_switch_drop + he355_multiply_plain by NTT(A + B J) + he355_add per term, he355_add_plain, he355_rescale -- the way
            tools/ckks_eval_poly_probe.py drives the real call, whose device-slab oracle this one extends.
  codec     he355_ckks_encode_complex / he355_ckks_decode_complex per vector beside he355_ckks_encode / he355_ckks_decode, 64 vectors.
The shapes: ckks8192 (N = 8192 {60, 40 x 5, 60}) and headline (N = 2^15, L = 16), as tools/ckks_eval_poly_probe.py's.  The candidates
alternate inside one process, every one is warmed up first, and the figures are min / median / max over the regions
(tools/probe_common.py).  Keys and inputs are synthetic: nothing timed depends on what they hold.
Usage: python tools/ckks_complex_probe.py [regions] [calls per region] [all | ckks8192 | headline]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import ckks_complex_ref as cref
from tools.ckks_eval_poly_probe import SHAPES, Composed, Slab, calls, repeats, which
from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
SEPTIC = [0.3 + 0.01 * k + (0.1 - 0.02 * k) * 1j for k in range(8)]


class ComposedComplex(Composed):
    """Composed with a pair of residue rows per constant: the full plaintext [L][N] that holds pair[s(e)] at NTT index e"""

    def const(self, L, pair):
        key = (L, tuple(int(v) for v in pair[0]), tuple(int(v) for v in pair[1]))
        if key not in self.consts:
            self.consts[key] = self.g.to_device(cref.spread(pair, L, self.N))
        return self.consts[key]


def composed_tree(g, n, src, L, coeffs, log_baby, scale):
    o = ComposedComplex(g, n)
    o.N, o.ntt = g.N, None
    ev = cref.Evaluator.__new__(cref.Evaluator)
    cref.real.Evaluator.__init__(ev, o, [1.0 if c != 0 else 0.0 for c in cref.trimmed(coeffs)], log_baby, L, scale, scale, None)
    ev.p, ev.u, ev._ccombine = cref.trimmed(coeffs), g.ckks_complex_unit(L), o.combine
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
    q = g.moduli
    slabs = [g.alloc(n * per) for _ in range(8)]  # eight distinct slabs: every term's bytes come from HBM
    for k, b in enumerate(slabs):
        g.fill_uniform(b, n * 2 * L, list(range(L)), 20 + k)
    out = g.alloc(n * per)
    fs, T = [lambda: g.add(L, 2, n, slabs[0], slabs[1], be.Context.pairwise(), out)], (2, 4, 8)
    for t in T:
        terms = [(slabs[k], L) for k in range(t)]
        a0 = [[(12345 + 977 * k + i) % q[i] for i in range(L)] for k in range(t)]
        a1 = [[(54321 + 613 * k + i) % q[i] for i in range(L)] for k in range(t)]
        cst = [q[i] - 1 for i in range(L)]
        fs.append(lambda terms=terms, a0=a0, cst=cst: g.combine_scalars(L, 2, n, terms, a0, out, cst))
        fs.append(lambda terms=terms, a0=a0, a1=a1, cst=cst: g.combine_scalars_complex(L, 2, n, terms, list(zip(a0, a1)), out, [cst, cst]))
    ts = alternated(g, fs, [calls * 4] * len(fs), repeats)
    print(f"   rate   k_addsub {fmt(ts[0])} us = {3 * n * per * 8 / ts[0][1] / 1e6:6.2f} TB/s", flush=True)
    for k, t in enumerate(T):
        tr, tc = ts[1 + 2 * k], ts[2 + 2 * k]
        print(f"   rate   {t} terms  k_scalar_combine {fmt(tr)} us = {(t + 1) * n * per * 8 / tr[1] / 1e6:6.2f} TB/s   k_scalar_combine_cplx {fmt(tc)} us = "
              f"{(t + 1) * n * per * 8 / tc[1] / 1e6:6.2f} TB/s   cplx / real {tc[1] / tr[1]:5.3f}", flush=True)
    if L >= 4:
        pl = g.ckks_eval_poly_complex_plan(L, SEPTIC, 1, scale, scale, n)
        tree, ev = composed_tree(g, n, slabs[0], L, SEPTIC, 1, scale)
        tc, tt = alternated(g, [lambda: g.ckks_eval_poly_complex(L, n, slabs[0], SEPTIC, 1, scale, scale, out), tree], [calls] * 2, repeats, warmup=1)
        print(f"   call   degree 7: depth {pl['depth']}, {pl['products']} products, {pl['combinations']} combinations   he355_ckks_eval_poly_complex {fmt(tc)}   "
              f"composed {fmt(tt)}   composed / call {tt[1] / tc[1]:5.2f}", flush=True)
    # the codec, 64 vectors of N / 2 slots
    half, Lt = N // 2, g.L
    rng = np.random.default_rng(1)
    vr, vc = g.to_device(rng.uniform(-1, 1, (n, half)).view(np.uint64)), g.to_device(rng.uniform(-0.7, 0.7, (n, half, 2)).view(np.uint64))
    plain, dr, dc = g.alloc(n * Lt * N), g.alloc(n * half), g.alloc(n * half * 2)
    g.ckks_encode_complex(n, vc, half, scale, plain)
    Ld = min(Lt, 16)
    te, tec, td, tdc = alternated(g, [lambda: g.ckks_encode(n, vr, half, scale, plain), lambda: g.ckks_encode_complex(n, vc, half, scale, plain),
                                      lambda: g.ckks_decode(Ld, n, plain, scale, dr), lambda: g.ckks_decode_complex(Ld, n, plain, scale, dc)], [calls] * 4, repeats)
    per_vec = lambda t: " / ".join(f"{v / n:8.2f}" for v in t)
    print(f"   codec  us per vector: encode {per_vec(te)}   encode_complex {per_vec(tec)}   ratio {tec[1] / te[1]:5.3f}", flush=True)
    print(f"   codec  us per vector: decode {per_vec(td)}   decode_complex {per_vec(tdc)}   ratio {tdc[1] / td[1]:5.3f}   (L = {Ld})", flush=True)
    print(f"   he355_poly_stats: {g.poly_stats()}", flush=True)
    g.close()


if __name__ == "__main__":
    for name in ("ckks8192", "headline"):
        if which in ("all", name):
            run(name)
