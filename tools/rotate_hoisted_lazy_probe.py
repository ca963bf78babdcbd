#!/usr/bin/env python3
"""The lazy-mod-down plain sum against the eager one, on one MI355X: ONE he355_rotate_hoisted_plain_sum_lazy call over R steps against ONE
he355_rotate_hoisted_plain_sum call over the same steps and slab, R = 1, 2, 4, 8, 16, n = 64, for
  bfv8192     BFV  N = 8192 {60,40,60}, NTT form
  ckks16384   CKKS N = 16384 {60,45,45,45,60} (L = 4)
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain)
The eager call is unchanged code: it is the yardstick.  The crossover R is the first R at which the lazy call's median is below the eager
call's.  `rate`: the accumulate kernel's identity form alone (the lazy sum of the identity, k_hoist_acc_qp<false>: a ciphertext slab and one
plaintext read, a slab written) beside k_addsub (he355_add of two different slabs: two read, one written), as bytes moved per second; the
keyed form cannot be called without its key product and is not timed alone.
The candidates alternate inside one process, every shape is warmed up first (which also builds the permuted keys), and the figures are
min / median / max over the regions (tools/probe_common.py).  Keys and plaintexts are synthetic (uniform residues): nothing timed depends
on what they hold.
Usage: python tools/rotate_hoisted_lazy_probe.py [regions] [calls per region] [all | bfv8192 | ckks16384 | headline]"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
which = sys.argv[3] if len(sys.argv) > 3 else "all"
RS = (1, 2, 4, 8, 16)
SHAPES = {
    "bfv8192": (be.SCHEME_BFV, 8192, [60, 40, 60]),
    "ckks16384": (be.SCHEME_CKKS, 16384, [60, 45, 45, 45, 60]),
    "headline": (be.SCHEME_CKKS, 32768, be.chain_bits(16, 45)),
}


def run(name, n=64):
    scheme, N, bits = SHAPES[name]
    bfv = scheme == be.SCHEME_BFV
    g = be.Context(scheme, N, bit_sizes=bits, plain_bits=20 if bfv else 0, sec128=False, device=0)
    L, K = g.L, g.K
    per = 2 * L * N
    steps = list(range(1, max(RS) + 1))
    for k, s in enumerate(steps):
        g.set_galois_key_synthetic(g.galois_elt(s), 100 + k)
    print(f"== {name}: N = {N} {bits if len(bits) < 8 else '{60, 45 x 15, 60}'}  L = {L}  n = {n}  ({'BFV, NTT form' if bfv else 'CKKS'})", flush=True)
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls")
    R = max(RS)
    src, out, other = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    pts, pts_qp = g.alloc(R * L * N), g.alloc(R * (L + 1) * N)
    g.fill_uniform(src, n * 2 * L, list(range(L)), 7)
    g.fill_uniform(other, n * 2 * L, list(range(L)), 8)
    g.fill_uniform(pts, R * L, list(range(L)), 9)
    g.fill_uniform(pts_qp, R * (L + 1), list(range(L)) + [K - 1], 9)
    cross = None
    for R in RS:
        def lazy():
            g.rotate_hoisted_plain_sum_lazy(L, n, src, steps[:R], pts_qp, out)

        def eager():
            g.rotate_hoisted_plain_sum(L, n, src, steps[:R], pts, out)

        tl, te = alternated(g, [lazy, eager], [calls] * 2, repeats)
        if cross is None and tl[1] < te[1]:
            cross = R
        print(f"   R = {R:2d}  lazy {fmt(tl)}   eager {fmt(te)}   eager / lazy {te[1] / tl[1]:5.2f}", flush=True)
    print(f"   the lazy sum wins from R = {cross} on" if cross else "   the lazy sum loses at every R measured", flush=True)

    def acc():
        g.rotate_hoisted_plain_sum_lazy(L, n, src, [0], pts_qp, out)

    def add():
        g.add(L, 2, n, src, other, be.Context.pairwise(), out)

    tf, ta = alternated(g, [acc, add], [calls * 4] * 2, repeats)
    bf, ba = (2 * n * per + L * N) * 8, 3 * n * per * 8  # a slab read, one written, the one plaintext; two slabs read, one written
    print(f"   rate: k_hoist_acc_qp<identity> {fmt(tf)} us = {bf / tf[1] / 1e6:7.2f} TB/s   k_addsub {fmt(ta)} us = {ba / ta[1] / 1e6:7.2f} TB/s", flush=True)
    st = g.hoist_stats()
    print(f"   digit lifts {st['digit_lifts']}, key products {st['key_products']}, mod-downs {st['mod_downs']}", flush=True)
    g.close()


for name in SHAPES:
    if which in ("all", name):
        run(name)
