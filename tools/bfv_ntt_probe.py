#!/usr/bin/env python3
"""The NTT-form BFV plaintext inner product on the device, out(i, j) = sum_k ct(i, k) (.) pt(k, j), for N = 8192 {60,40,60} (L = 2) and
N = 32768 {60,40,40,60} (L = 3), size 2, shapes rows x cols x inner = 1 x 64 x 256, 16 x 16 x 64, 1 x 1 x 1024.  Three ways to the same sum:
(a) he355_bfv_multiply_plain_accumulate: one launch of k_bfv_plain_mac;
(b) the unfused loop of the NTT-form calls: per inner index one he355_bfv_multiply_plain_ntt over the rows x cols results and one he355_add;
(c) what the library offered before the NTT-form calls: per inner index one he355_bfv_multiply_plain in coefficient form (a forward and
    an inverse transform per result polynomial and term) and one he355_add.
The three alternate inside one process (a, b, c, a, b, c, ...), every region is HIP-event timed on the context's stream (he355_timer_begin /
_end), every shape is warmed up first, and the figures are min / median / max over the regions.  (a) and (b) are compared bit for bit
before anything is timed.  The HBM share of (a) is its compulsory bytes -- every operand word read once, every result word written once --
over its time; he355_add over a slab of the same order is timed beside it (k_addsub: the streaming kernel DESIGN.md 5.4 measures).
`fused`: (a) alone (the A/B of two builds of the library, HE355_LIB_PATH: one process each, alternated by the caller).
`kernels`: a few calls of (a) and one of (b) per shape and nothing else, for a profiler run of its own
(rocprofv3 --kernel-trace --stats -- python tools/bfv_ntt_probe.py 3 1 kernels; counters: a second run with --pmc).
Usage: python tools/bfv_ntt_probe.py [regions] [scale of the calls per region] [all | fused | kernels]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.probe_common import alternated

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
mode = sys.argv[3] if len(sys.argv) > 3 else "all"
SIZE = 2
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
SHAPES = ((1, 64, 256), (16, 16, 64), (1, 1, 1024))


def shape_run(g, N, L, rows, cols, inner):
    n, per = rows * cols, SIZE * L * N
    # ciphertext (i, k) at k * rows + i, plaintext (k, j) at k * cols + j: the layout whose terms of one k the Indexer addresses in one call
    ctn, ptn, out_a, out_b, tmp = g.alloc(inner * rows * per), g.alloc(inner * cols * L * N), g.alloc(n * per), g.alloc(n * per), g.alloc(n * per)
    g.fill_uniform(ctn, inner * rows * SIZE * L, list(range(L)), 1)
    g.fill_uniform(ptn, inner * cols * L, list(range(L)), 2)
    # coefficient-form operands of (c): uniform residues as ciphertexts, one encoded slot value per plaintext
    ctc, plc = g.alloc(inner * rows * per), g.alloc(inner * cols * N)
    g.fill_uniform(ctc, inner * rows * SIZE * L, list(range(L)), 3)
    vals = g.to_device(np.arange(1, inner * cols + 1, dtype=np.int64).view(np.uint64))
    g.bfv_encode(inner * cols, vals, 1, plc)
    out_c = g.alloc(n * per)

    def fused():
        g.bfv_multiply_plain_accumulate(L, SIZE, rows, cols, inner, ctn, 1, rows, ptn, cols, 1, out_a)

    def loop(mul, ct, pt, out):
        for k in range(inner):
            ix = be.Context.outer(k * rows, rows, k * cols, cols)
            mul(L, SIZE, n, ct, pt, ix, out if k == 0 else tmp)
            if k:
                g.add(L, SIZE, n, out, tmp, be.Context.pairwise(), out)

    unfused = lambda: loop(g.bfv_multiply_plain_ntt, ctn, ptn, out_b)
    parent = lambda: loop(g.bfv_multiply_plain, ctc, plc, out_c)
    fused()
    unfused()
    same = np.array_equal(out_a.download_head((min(n, 4) * per,)), out_b.download_head((min(n, 4) * per,)))
    tail = np.array_equal(out_a.download_range((n - 1) * per, (per,)), out_b.download_range((n - 1) * per, (per,)))
    if not (same and tail):
        raise SystemExit(f"N {N} shape {rows}x{cols}x{inner}: the fused call and the unfused loop differ")
    words = (inner * rows * SIZE + inner * cols + n * SIZE) * L * N
    if mode == "kernels":
        for _ in range(repeats):
            fused()
        unfused()
        g.sync()
        print(f"N = {N} L = {L}  {rows} x {cols} x {inner}: compulsory bytes of the fused call {words * 8}", flush=True)
    elif mode == "fused":
        (ta,) = alternated(g, [fused], [max(1, scale * min(20, (1 << 34) // (words * 8)))], repeats)
        print(f"N = {N} L = {L}  {rows} x {cols} x {inner}  (a) fused accumulate {ta[0]:11.1f} / {ta[1]:11.1f} / {ta[2]:11.1f} us -> {words * 8 / ta[1] / 1e6:6.3f} TB/s", flush=True)
    else:
        ca = max(1, scale * min(20, (1 << 34) // (words * 8)))
        ta, tb, tc = alternated(g, [fused, unfused, parent], [ca, scale, scale], repeats)
        f = lambda t: " / ".join(f"{v:11.1f}" for v in t)
        terms = n * inner
        print(f"N = {N} L = {L}  rows x cols x inner = {rows} x {cols} x {inner}   us per call, min / median / max of {repeats} regions")
        print(f"  (a) fused accumulate              {f(ta)}   per result {ta[1] / n:9.2f}  per term {ta[1] / terms:8.4f}")
        print(f"  (b) multiply_plain_ntt + add loop {f(tb)}   per result {tb[1] / n:9.2f}  per term {tb[1] / terms:8.4f}   (b) / (a) {tb[1] / ta[1]:7.2f}")
        print(f"  (c) multiply_plain + add loop     {f(tc)}   per result {tc[1] / n:9.2f}  per term {tc[1] / terms:8.4f}   (c) / (a) {tc[1] / ta[1]:7.2f}")
        print(f"  (a) compulsory bytes {words * 8} -> {words * 8 / ta[1] / 1e6:6.3f} TB/s at the median ({words * 8 / ta[0] / 1e6:6.3f} at the fastest region)"
              f" = {words * 8 / ta[1] / 1e6 / 8.0 * 100:5.1f} % of the 8 TB/s peak", flush=True)
    for b in (ctn, ptn, out_a, out_b, tmp, ctc, plc, vals, out_c):
        b.free()


def addsub_rate(g, N, L):
    """he355_add over slabs of 512 MiB of size-2 ciphertexts: two slabs read, one written"""
    per = SIZE * L * N
    n = max(1, (1 << 29) // (per * 8))
    a, b, o = (g.alloc(n * per) for _ in range(3))
    g.fill_uniform(a, n * SIZE * L, list(range(L)), 5)
    g.fill_uniform(b, n * SIZE * L, list(range(L)), 6)
    f = lambda: g.add(L, SIZE, n, a, b, be.Context.pairwise(), o)
    (t,) = alternated(g, [f], [10 * scale], repeats)
    print(f"N = {N} L = {L}  he355_add over {n} ciphertexts ({3 * n * per * 8} bytes): {t[0]:9.1f} / {t[1]:9.1f} / {t[2]:9.1f} us -> {3 * n * per * 8 / t[1] / 1e6:6.3f} TB/s"
          f" at the median", flush=True)
    for x in (a, b, o):
        x.free()


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    L = g.L
    print(f"== N = {N} {bits}  L = {L}  size {SIZE}  fp64-engine primes {[i for i in range(L) if g.fp64[i]]}", flush=True)
    for rows, cols, inner in SHAPES:
        shape_run(g, N, L, rows, cols, inner)
    if mode == "all":
        addsub_rate(g, N, L)
    g.close()
