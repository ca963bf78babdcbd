#!/usr/bin/env python3
"""The baby-step/giant-step linear transform against the flat lazy plain sum, on one MI355X: ONE he355_linear_transform_bsgs call against ONE
he355_rotate_hoisted_plain_sum_lazy call over the same R = n1 n2 steps 0 .. R - 1 and the same slab, n = 64, for
  bfv8192     BFV  N = 8192 {60,40,60}, NTT form
  ckks16384   CKKS N = 16384 {60,45,45,45,60} (L = 4)
  headline    CKKS N = 2^15, L = 16 (DESIGN.md 5.1's chain)
and the splits (baby x giant) 2 x 2, 4 x 4, 8 x 8, 16 x 4 and 4 x 16.  The flat call is unchanged code: it is the yardstick.  Also printed:
the key bytes the permuted copies hold after each route alone (he355_hoist_stats.key_bytes, after he355_hoist_release_keys), the scratch
bound of the call, and `rate`: the inner-sum kernel alone as the DIFFERENCE of two calls over eight identity babies, with two identity giant
rows and with one -- the second row is one more k_bsgs_inner launch in its accumulate form: eight store slots, eight plaintexts and the
accumulator read, the accumulator written -- beside k_addsub (he355_add of two different slabs: two read, one written), as bytes moved per
second.
The candidates alternate inside one process, every shape is warmed up first (which also builds the permuted keys), and the figures are
min / median / max over the regions (tools/probe_common.py).  Keys and plaintexts are synthetic (uniform residues): nothing timed depends
on what they hold.
Usage: python tools/linear_transform_bsgs_probe.py [regions] [calls per region] [all | bfv8192 | ckks16384 | headline]"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
which = sys.argv[3] if len(sys.argv) > 3 else "all"
SPLITS = ((2, 2), (4, 4), (8, 8), (16, 4), (4, 16))  # (n_baby, n_giant)
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
    R_max = max(a * b for a, b in SPLITS)
    for s in range(1, R_max):
        g.set_galois_key_synthetic(g.galois_elt(s), 100 + s)
    print(f"== {name}: N = {N} {bits if len(bits) < 8 else '{60, 45 x 15, 60}'}  L = {L}  n = {n}  ({'BFV, NTT form' if bfv else 'CKKS'})", flush=True)
    print(f"   us per call, min / median / max of {repeats} regions of {calls} calls")
    src, out, other = g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    pts_qp = g.alloc(R_max * (L + 1) * N)
    g.fill_uniform(src, n * 2 * L, list(range(L)), 7)
    g.fill_uniform(other, n * 2 * L, list(range(L)), 8)
    g.fill_uniform(pts_qp, R_max * (L + 1), list(range(L)) + [K - 1], 9)
    wins = []
    for nb, ng in SPLITS:
        R = nb * ng
        baby, giant, flat = list(range(nb)), [nb * j for j in range(ng)], list(range(R))

        def bsgs():
            g.linear_transform_bsgs(L, n, src, baby, giant, pts_qp, out)

        def lazy():
            g.rotate_hoisted_plain_sum_lazy(L, n, src, flat, pts_qp, out)

        held = []
        for f in (bsgs, lazy):  # the key bytes of each route alone
            g.hoist_release_keys()
            f()
            g.sync()
            held.append(g.hoist_stats()["key_bytes"])
        tb, tl = alternated(g, [bsgs, lazy], [calls] * 2, repeats, warmup=1)
        if tb[1] < tl[1]:
            wins.append(f"{nb} x {ng}")
        print(f"   R = {R:2d} as {nb:2d} x {ng:2d}  bsgs {fmt(tb)}   flat lazy {fmt(tl)}   flat / bsgs {tl[1] / tb[1]:5.2f}   "
              f"key bytes {held[0] / 2 ** 20:8.0f} / {held[1] / 2 ** 20:8.0f} MiB   scratch bound {g.linear_transform_bsgs_scratch_bytes(L, n, nb) / 2 ** 20:7.0f} MiB", flush=True)
    print(f"   the transform is faster than the flat sum at: {', '.join(wins) if wins else 'no split measured'}", flush=True)

    eight = [0] * 8

    def one_row():
        g.linear_transform_bsgs(L, n, src, eight, [0], pts_qp, out)

    def two_rows():
        g.linear_transform_bsgs(L, n, src, eight, [0, 0], pts_qp, out)

    def add():
        g.add(L, 2, n, src, other, be.Context.pairwise(), out)

    t1, t2, ta = alternated(g, [one_row, two_rows, add], [calls * 2] * 3, repeats)
    qp = n * 2 * (L + 1) * N  # words of a chunk's Q P block
    bi, ba = (8 * qp + 8 * (L + 1) * N + 2 * qp) * 8, 3 * n * per * 8
    dt = t2[1] - t1[1]
    print(f"   rate: k_bsgs_inner (8 terms, accumulate) {dt:9.1f} us (medians {t2[1]:.1f} - {t1[1]:.1f}) = {bi / dt / 1e6:7.2f} TB/s   "
          f"k_addsub {fmt(ta)} us = {ba / ta[1] / 1e6:7.2f} TB/s", flush=True)
    st = g.hoist_stats()
    print(f"   digit lifts {st['digit_lifts']}, key products {st['key_products']}, mod-downs {st['mod_downs']}, inner sums {st['inner_sums']}", flush=True)
    g.close()


for name in SHAPES:
    if which in ("all", name):
        run(name)
