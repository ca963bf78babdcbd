#!/usr/bin/env python3
"""The CKKS modulus raise on one MI355X:
  call      ONE he355_ckks_mod_raise (size 2, L_in = 1) against the composition it is defined by, through the public calls -- the copy of row 0
            (he355_mod_switch_drop to level 1: one launch for the batch), he355_ntt_inverse, he355_ckks_lift_centred, he355_ntt_forward -- at
            n = 1, 8 and 64.  The traffic count: the composition moves about 5 L + 7 slabs per polynomial, the fused route about 3 L + 3.
  split     n = 1 with the targets of a column dealt to blocks (the rule) and without (he355_set_latency_max(0)).
  rate      k_raise_lift (he355_ckks_lift_centred: one launch, 1 + L slabs) beside k_addsub (he355_add of two slabs: 3 slabs) in the same run,
            in bytes moved, and the fused call at its own traffic count (3 L + 3 slabs: the copy 2, the inverse row pass 2, k_raise_cols
            1 + (L - 1), the forward row pass 2 (L - 1)).  k_raise_cols alone is taken from a kernel trace of `trace` mode:
            rocprofv3 --kernel-trace --stats -- python tools/ckks_mod_raise_probe.py trace <shape>
The shapes:
  ckks8192    CKKS N = 8192 {60, 40 x 5, 60}   raising 1 -> 6
  ckks16384   CKKS N = 16384 {60, 45 x 5, 60}  raising 1 -> 6
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain), raising 1 -> 16
The candidates alternate inside one process, every one is warmed up first, and the figures are min / median / max over the regions
(tools/probe_common.py).  The inputs are synthetic (uniform residues): nothing timed depends on what they hold.
Usage: python tools/ckks_mod_raise_probe.py [regions] [calls per region] [all | ckks8192 | ckks16384 | headline]
       python tools/ckks_mod_raise_probe.py trace [shape]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
repeats = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 and not trace else 4
which = (sys.argv[2] if len(sys.argv) > 2 else "headline") if trace else (sys.argv[3] if len(sys.argv) > 3 else "all")
SHAPES = {
    "ckks8192": (8192, [60, 40, 40, 40, 40, 40, 60]),
    "ckks16384": (16384, [60, 45, 45, 45, 45, 45, 60]),
    "headline": (32768, be.chain_bits(16, 45)),
}
SIZE = 2


def run(name):
    N, bits = SHAPES[name]
    g = be.Context(be.SCHEME_CKKS, N, bit_sizes=bits, sec128=False, device=0)
    L = g.L
    n_max = 64
    polys = n_max * SIZE
    print(f"== {name}: N = {N} {bits if len(bits) < 10 else '{60, 45 x 15, 60}'}  raising 1 -> {L}, size {SIZE}", flush=True)
    src, out, other = g.alloc(polys * N), g.alloc(polys * L * N), g.alloc(polys * L * N)
    tmp = g.alloc(polys * N)
    g.fill_uniform(src, polys, [0], 7)
    g.fill_uniform(other, polys * L, list(range(L)), 8)
    g.fill_uniform(out, polys * L, list(range(L)), 9)

    def fused(n):
        return lambda: g.ckks_mod_raise(1, L, SIZE, n, src, out)

    def composed(n):
        def f():
            g.mod_switch_drop(1, 1, n * SIZE, src, tmp)  # the copy of row 0, one launch
            g.ntt(tmp, n * SIZE, [0], inverse=True)
            g.ckks_lift_centred(L, n * SIZE, tmp, out)
            g.ntt(out, n * SIZE * L, list(range(L)))
        return f

    if trace:
        for _ in range(6):
            fused(n_max)()
            composed(n_max)()
            g.add(L, SIZE, n_max, out, other, be.Context.pairwise(), out)
        g.sync()
        print(f"   trace: 6 x (fused, composed, add) at n = {n_max}; slab = {polys * N * 8} bytes, L = {L}: {g.raise_stats()}", flush=True)
        g.close()
        return
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls")
    for n in (1, 8, 64):
        tf, tc = alternated(g, [fused(n), composed(n)], [calls] * 2, repeats)
        slab = n * SIZE * N * 8
        print(f"   call   n = {n:2d}: he355_ckks_mod_raise {fmt(tf)}   composed {fmt(tc)}   composed / call {tc[1] / tf[1]:5.2f}   "
              f"call at 3L+3 slabs {(3 * L + 3) * slab / tf[1] / 1e6:5.2f} TB/s, composed at 5L+7 {(5 * L + 7) * slab / tc[1] / 1e6:5.2f} TB/s", flush=True)
    g.raise_stats(reset=True)
    g.set_latency_max(0)
    off = fused(1)
    off()
    assert g.raise_stats()["split_launches"] == 0
    g.set_latency_max(None)

    def unsplit():
        g.set_latency_max(0)
        off()
        g.set_latency_max(None)

    ts, tu = alternated(g, [fused(1), unsplit], [calls] * 2, repeats)
    print(f"   split  n =  1: with the target split {fmt(ts)}   without {fmt(tu)}   without / with {tu[1] / ts[1]:5.2f}", flush=True)
    slab = polys * N * 8

    def add():
        g.add(L, SIZE, n_max, out, other, be.Context.pairwise(), out)

    def lift():
        g.ckks_lift_centred(L, polys, src, out)

    ta, tl = alternated(g, [add, lift], [calls * 2] * 2, repeats)
    print(f"   rate   k_addsub {fmt(ta)} us = {3 * L * slab / ta[1] / 1e6:6.2f} TB/s of 3 L slabs", flush=True)
    print(f"   rate   k_raise_lift {fmt(tl)} us = {(1 + L) * slab / tl[1] / 1e6:6.2f} TB/s of 1 + L slabs", flush=True)
    print(f"   he355_raise_stats: {g.raise_stats()}", flush=True)
    g.close()


for name in SHAPES:
    if which in ("all", name):
        run(name)
