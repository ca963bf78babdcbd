#!/usr/bin/env python3
"""The BFV noise budget on the device (he355_bfv_noise_budget), for N = 8192 {60,40,60} and N = 32768 {60,40,40,60}:
(a) us per ciphertext against he355_decrypt of the same slab (size 2, batch 1, 64 and 1024): the two sides alternate inside one process,
    every region is HIP-event timed on the context's stream (he355_timer_begin / _end), every shape is warmed up first, and the figure is
    the median of the repeats (min and max beside it);
(b) the budget after each stage of the bfv_matmul-style chain with real keys at the reference's default t (20 bits): fresh -> multiply
    -> relinearize -> rotate_sum (the 127 steps of the 128 x 128 MatMultRow) -> bfv_mod_switch to every lower level, and the same switch
    applied BEFORE the rotations (switch, then rotate_sum at the lower level): the lowest level the rotation chain can run at.
    The smallest budget over the batch is printed; where it is positive the decryption is checked against the expected slots.
(c) `kernels`: a few batch-1024 calls at W = 5 (N = 32768, 3 data primes) and W = 18 (N = 1024, 16 data primes) and nothing else, for a
    profiler run of its own (rocprofv3 --kernel-trace --stats -- python tools/bfv_noise_probe.py 10 7 2 kernels).
Usage: python tools/bfv_noise_probe.py [calls per region] [repeats] [table batch] [all | time | table | kernels]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle as ho  # keys and the slot codec only: nothing timed goes through it
from tools.probe_common import alternated, region

be = importlib.import_module("reference-seal-backend_amd")
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
tab_batch = int(sys.argv[3]) if len(sys.argv) > 3 else 2
mode = sys.argv[4] if len(sys.argv) > 4 else "all"
SIZE = 2


def timing(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    g.set_secret_key(o.keygen_secret(1))
    L = g.L
    print(f"== (a) N = {N} {bits}  L = {L}  size {SIZE}: us per ciphertext, min / median / max of {repeats} regions", flush=True)
    lib = be.lib()
    for n in (1, 64, 1024):
        ct, dec, out = g.alloc(n * SIZE * L * N), g.alloc(n * N), g.alloc(n)
        g.fill_uniform(ct, n * SIZE * L, list(range(L)), 1)
        k = max(2, calls // (1 if n < 1024 else 4))
        bits_ptr = out.ptr.value + 4 * n
        tn, td = alternated(g, [lambda: lib.he355_bfv_noise_budget(g.h, L, SIZE, n, ct.ptr, out.ptr, bits_ptr), lambda: g.decrypt(L, SIZE, n, ct, dec)], [k, k], repeats, warmup=3)
        f = lambda t: " / ".join(f"{v / n:9.3f}" for v in t)
        print(f"batch {n:5d}  he355_bfv_noise_budget {f(tn)}   he355_decrypt {f(td)}   ratio of medians {tn[1] / td[1]:.3f}", flush=True)
        for b in (ct, dec, out):
            b.free()
    g.close()


def table(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    t, L, n = o.t, g.L, tab_batch
    codec = ho.BatchCodec(N, t)
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    g.keygen_relin(5)
    k = 0
    while (1 << k) < N // 2:  # the default Galois key set of bench.py's bfv_matmul: +-2^k row rotations
        for s in (1 << k, -(1 << k)):
            g.keygen_galois(g.galois_elt(s), 7)
        k += 1
    dim = 128
    sp = (N // 2) // dim
    steps = [j * sp for j in range(1, dim)]
    rng = np.random.default_rng(N)
    x, y = (rng.integers(-(t // 2), t // 2 + 1, (n, N)) for _ in range(2))
    enc = lambda v: np.stack([codec.encode(row) for row in v])
    cen = lambda v: np.where(v % t > t // 2, v % t - t, v % t).astype(np.int64)
    xy = cen(x.astype(object) * y.astype(object))
    half = N // 2
    rsum = np.zeros_like(xy, dtype=object)
    for j in range(dim):  # the result plus its 127 row rotations
        rsum = rsum + np.concatenate([np.roll(xy[:, :half], -j * sp, axis=1), np.roll(xy[:, half:], -j * sp, axis=1)], axis=1)
    rsum = cen(rsum)
    print(f"== (b) N = {N} {bits}  t = {t} ({t.bit_length()} bits)  batch {n}: stage, level, bits(q_L), noise_bits (max), budget (min), decrypts", flush=True)

    def show(tag, buf, size, Ls, want):
        budget, nb = g.bfv_noise_budget(Ls, size, n, buf, with_bits=True)
        dec, vals = g.alloc(n * N), g.alloc(n * N)
        g.decrypt(Ls, size, n, buf, dec)
        g.bfv_decode(n, dec, vals)
        ok = np.array_equal(vals.download().view(np.int64).reshape(n, N), want)
        qL = 1
        for q in g.moduli[:Ls]:
            qL *= int(q)
        print(f"{tag:<44} L {Ls}  bits(q_L) {qL.bit_length():4d}  noise_bits {int(nb.max()):4d}  budget {int(budget.min()):4d}  decrypts {'yes' if ok else 'NO'}", flush=True)
        dec.free()
        vals.free()

    cx, cy, c3, c2, acc = (g.alloc(n * s * L * N) for s in (2, 2, 3, 2, 2))
    g.encrypt(n, g.to_device(enc(x)), 11, 0, cx)
    g.encrypt(n, g.to_device(enc(y)), 11, n, cy)
    show("fresh", cx, 2, L, cen(x.astype(object)))
    g.bfv_multiply(L, n, cx, cy, be.Context.pairwise(), c3)
    show("multiply (size 3)", c3, 3, L, xy)
    g.relinearize(L, n, c3, c2)
    show("relinearize", c2, 2, L, xy)
    ks = g.rotate_sum(L, n, c2, steps, acc)
    show(f"rotate_sum ({len(steps)} steps, {ks} key switches)", acc, 2, L, rsum)
    for L_to in range(L - 1, 0, -1):
        low, lacc = g.alloc(n * 2 * L_to * N), g.alloc(n * 2 * L_to * N)
        g.bfv_mod_switch(L, L_to, 2, n, acc, low)
        show(f"  rotate_sum at {L}, then switch to {L_to}", low, 2, L_to, rsum)
        g.bfv_mod_switch(L, L_to, 2, n, c2, low)
        show(f"  switch to {L_to} before the rotations", low, 2, L_to, xy)
        g.rotate_sum(L_to, n, low, steps, lacc)
        show(f"  switch to {L_to}, then rotate_sum there", lacc, 2, L_to, rsum)
        low.free()
        lacc.free()
    g.close()


def kernels():
    """batch 1024, size 2: k_bfv_noise_bits<5> and <18> under a profiler; compulsory bytes per call printed for the rate"""
    for N, bits in ((32768, [60, 40, 40, 60]), (1024, [60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 59, 60])):
        g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
        o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
        g.set_secret_key(o.keygen_secret(1))
        L, n = g.L, 1024
        ct, out = g.alloc(n * SIZE * L * N), g.alloc(n)
        g.fill_uniform(ct, n * SIZE * L, list(range(L)), 1)
        f = lambda: be.lib().he355_bfv_noise_budget(g.h, L, SIZE, n, ct.ptr, out.ptr, None)
        for _ in range(3):
            f()
        g.sync()
        us = region(g, f, calls)
        print(f"W = {L + 2}  N = {N}  batch {n}: {us:10.1f} us per call; k_bfv_noise_bits reads 2 L N 8 = {2 * L * N * 8} bytes per ciphertext, "
              f"{n * 2 * L * N * 8} per call in {-(-n // min(1024, max(64, (1 << 21) // N)))} launches", flush=True)
        g.close()


RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
if mode in ("all", "time"):
    for N, bits in RINGS:
        timing(N, bits)
if mode in ("all", "table"):
    for N, bits in RINGS:
        table(N, bits)
if mode == "kernels":
    kernels()
