#!/usr/bin/env python3
"""Hoisted rotations against the ordinary ones, on one MI355X: ONE he355_apply_galois_hoisted call over R elements against R he355_apply_galois
calls on the same slab, R = 1, 2, 4, 8, 16, for
  bfv8192     BFV  N = 8192 {60,40,60}, coefficient form, n = 64 and 256
  ckks16384   CKKS N = 16384 {60,45,45,45,60} (L = 4), n = 64
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain), n = 64
and, at R = 16, he355_rotate_hoisted_plain_sum against he355_rotate + he355_multiply_plain + he355_add (the CKKS shapes).  `rate`: the
finishing kernel alone (the plain sum of the identity, k_hoist_finish_ntt<PLAIN>: a ciphertext slab and one plaintext read, a slab written) beside
k_addsub (he355_add of two different slabs: two read, one written), as bytes moved per second.
The candidates alternate inside one process, every shape is warmed up first (which also builds the permuted keys), and the figures are
min / median / max over the regions (tools/probe_common.py).  Keys are synthetic (uniform residues): nothing timed depends on what a key holds.
Usage: python tools/rotate_hoisted_probe.py [regions] [calls per region] [all | bfv8192 | ckks16384 | headline]"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.probe_common import At, alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
which = sys.argv[3] if len(sys.argv) > 3 else "all"
RS = (1, 2, 4, 8, 16)
SHAPES = {
    "bfv8192": (be.SCHEME_BFV, 8192, [60, 40, 60], (64, 256)),
    "ckks16384": (be.SCHEME_CKKS, 16384, [60, 45, 45, 45, 60], (64,)),
    "headline": (be.SCHEME_CKKS, 32768, be.chain_bits(16, 45), (64,)),
}


def run(name):
    scheme, N, bits, batches = SHAPES[name]
    bfv = scheme == be.SCHEME_BFV
    g = be.Context(scheme, N, bit_sizes=bits, plain_bits=20 if bfv else 0, sec128=False, device=0)
    L = g.L
    per = 2 * L * N
    steps = list(range(1, max(RS) + 1))
    elts = [g.galois_elt(s) for s in steps]
    for k, e in enumerate(elts):
        g.set_galois_key_synthetic(e, 100 + k)
    print(f"== {name}: N = {N} {bits if len(bits) < 8 else '{60, 45 x 15, 60}'}  L = {L}  ({'BFV, coefficient form' if bfv else 'CKKS'})", flush=True)
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls; a Galois key holds {g.L * 2 * g.K * N * 8} bytes, its permuted copy as much again")
    for n in batches:
        src, out = g.alloc(n * per), g.alloc(max(RS) * n * per)
        g.fill_uniform(src, n * 2 * L, list(range(L)), 7)
        cross = None
        for R in RS:
            def hoisted():
                g.apply_galois_hoisted(L, n, src, elts[:R], out, ntt_form=not bfv)

            def ordinary():
                for r in range(R):
                    g.apply_galois(L, n, src, elts[r], At(out, r * n * per))

            th, to = alternated(g, [hoisted, ordinary], [calls] * 2, repeats)
            if cross is None and th[1] < to[1]:
                cross = R
            print(f"   n = {n:3d} R = {R:2d}  hoisted {fmt(th)}   {R} x apply_galois {fmt(to)}   ordinary / hoisted {to[1] / th[1]:5.2f}", flush=True)
        print(f"   n = {n}: hoisting wins from R = {cross} on" if cross else f"   n = {n}: hoisting loses at every R measured", flush=True)
        if not bfv:
            R = max(RS)
            pts, acc, rot, term = g.alloc(R * L * N), g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
            g.fill_uniform(pts, R * L, list(range(L)), 9)
            bcast = be.Context.outer(0, n, 0, 1)  # every ciphertext times the one plaintext

            def plain_sum():
                g.rotate_hoisted_plain_sum(L, n, src, steps[:R], pts, acc)

            def composed():
                for r in range(R):
                    g.rotate(L, n, src, steps[r], rot)
                    g.multiply_plain(L, 2, n, rot, At(pts, r * L * N), bcast, term if r else acc)
                    if r:
                        g.add(L, 2, n, acc, term, be.Context.pairwise(), acc)

            tp, tc = alternated(g, [plain_sum, composed], [calls] * 2, repeats)
            print(f"   n = {n:3d} R = {R:2d}  plain sum {fmt(tp)}   rotate + multiply_plain + add {fmt(tc)}   composed / hoisted {tc[1] / tp[1]:5.2f}", flush=True)

            def finish():
                g.rotate_hoisted_plain_sum(L, n, src, [0], pts, acc)

            def add():
                g.add(L, 2, n, src, rot, be.Context.pairwise(), term)

            tf, ta = alternated(g, [finish, add], [calls * 4] * 2, repeats)
            bf, ba = (2 * n * per + L * N) * 8, 3 * n * per * 8  # a slab read, one written, the one plaintext; two slabs read, one written
            print(f"   rate: k_hoist_finish_ntt<PLAIN> {fmt(tf)} us = {bf / tf[1] / 1e6:7.2f} TB/s   k_addsub {fmt(ta)} us = {ba / ta[1] / 1e6:7.2f} TB/s", flush=True)
            for b in (pts, acc, rot, term):
                b.free()
        src.free()
        out.free()
    st = g.hoist_stats()
    print(f"   permuted keys built {st['keys_permuted']}, holding {st['key_bytes']} bytes", flush=True)
    g.close()


for name in SHAPES:
    if which in ("all", name):
        run(name)
