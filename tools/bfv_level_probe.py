#!/usr/bin/env python3
"""BFV level operations on the device: us per call and achieved compulsory bytes/s of he355_bfv_mod_switch (L -> L-1 and L -> 1),
he355_bfv_add_plain and he355_bfv_multiply_plain at batch 1, 64 and 1024, for N = 32768 {60,40,40,60} and N = 8192 {60,40,60}; the
transform yardstick of multiply_plain (he355_ntt_forward + he355_ntt_inverse on the same polynomials, same run); and the use case:
he355_rotate_sum with the bfv_matmul configuration's steps at the top level against he355_bfv_mod_switch to one level less followed
by the same he355_rotate_sum there.  HIP-event timing on the context's stream (he355_timer_begin / _end: the end event is synchronised
inside the region), warm-up first, every figure repeated: min / median / max of the repeats.
Usage: python tools/bfv_level_probe.py [reps] [repeats] [rotate_batch]"""
import importlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
be = importlib.import_module("reference-seal-backend_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rot_batch = int(sys.argv[3]) if len(sys.argv) > 3 else 16
SIZE = 2


def timed(g, f, n_calls):
    """us per call: min, median, max over `repeats` timed regions of n_calls calls each, after a warm-up"""
    for _ in range(3):
        f()
    g.sync()
    us = []
    for _ in range(repeats):
        g.timer_begin()
        for _ in range(n_calls):
            f()
        us.append(g.timer_end() / n_calls * 1e3)
    return min(us), statistics.median(us), max(us)


def report(tag, n, t, nbytes=None, extra=""):
    lo, med, hi = t
    rate = f"  {nbytes / (med * 1e-6) / 1e12:6.3f} TB/s compulsory" if nbytes else ""
    print(f"{tag:<46} batch {n:5d}  us/call min {lo:10.1f} median {med:10.1f} max {hi:10.1f}{rate}{extra}", flush=True)


for N, bits in ((32768, [60, 40, 40, 60]), (8192, [60, 40, 60])):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    L = g.L
    print(f"== N = {N} {bits}  L = {L}  t = {g.t}  ciphertext size {SIZE}", flush=True)
    for n in (1, 64, 1024):
        ct = g.alloc(n * SIZE * L * N)
        out = g.alloc(n * SIZE * L * N)
        pt = g.alloc(n * N)
        g.fill_uniform(ct, n * SIZE * L, list(range(L)), 1)
        base = np.random.default_rng(n).integers(0, g.t, min(n, 64) * N, dtype=np.uint64)  # plaintexts: uniform mod t (64 distinct ones, tiled)
        pt.upload(np.tile(base, n // min(n, 64)))
        pw = be.Context.pairwise()
        word = 8
        poly = N * word
        k = 1 if n == 1024 else 4
        r = max(2, reps // k)
        if L >= 2:
            report(f"bfv_mod_switch L {L} -> {L - 1}", n, timed(g, lambda: g.bfv_mod_switch(L, L - 1, SIZE, n, ct, out), r), n * SIZE * (L + L - 1) * poly)
            report(f"bfv_mod_switch L {L} -> 1", n, timed(g, lambda: g.bfv_mod_switch(L, 1, SIZE, n, ct, out), r), n * SIZE * (L + 1) * poly)
        # add_plain out of place: every polynomial read and written, the plaintext read; in place: c0 read and written, the plaintext read
        report("bfv_add_plain (out of place)", n, timed(g, lambda: g.bfv_add_plain(L, SIZE, n, ct, pt, pw, out), r), n * (2 * SIZE * L + 1) * poly)
        report("bfv_add_plain (in place)", n, timed(g, lambda: g.bfv_add_plain(L, SIZE, n, out, pt, pw, out), r), n * (2 * L + 1) * poly)
        # multiply_plain: compulsory = ciphertext in, ciphertext out, plaintext in
        tm = timed(g, lambda: g.bfv_multiply_plain(L, SIZE, n, ct, pt, pw, out), r)
        report("bfv_multiply_plain (pairwise)", n, tm, n * (2 * SIZE * L + 1) * poly, f"  {tm[1] / (n * SIZE * L):8.3f} us/polynomial")
        if n >= 64:
            to = timed(g, lambda: g.bfv_multiply_plain(L, SIZE, n, ct, pt, be.Context.outer(0, n, 0, 1), out), r)
            report("bfv_multiply_plain (one plaintext)", n, to, n * 2 * SIZE * L * poly + poly, f"  {to[1] / (n * SIZE * L):8.3f} us/polynomial")
        # the yardstick: forward + inverse transform (k_cols_fwd + k_rows_fwd + k_rows_inv + k_cols_inv) of the same polynomials, in place

        def both():
            g.ntt(out, n * SIZE * L, list(range(L)))
            g.ntt(out, n * SIZE * L, list(range(L)), inverse=True)
        tt = timed(g, both, r)
        report("ntt_forward + ntt_inverse (yardstick)", n, tt, None, f"  {tt[1] / (n * SIZE * L):8.3f} us/polynomial")
        for b in (ct, out, pt):
            b.free()
    # the use case: rotate_sum with the bfv_matmul steps at L, against mod_switch to L - 1 + the same rotate_sum at L - 1
    if L >= 2:
        n = rot_batch
        dim = 128
        steps = [j * ((N // 2) // dim) for j in range(1, dim)]
        k = 0
        while (1 << k) < N // 2:
            for s in (1 << k, -(1 << k)):
                g.set_galois_key_synthetic(g.galois_elt(s), 100 + 2 * k + (s < 0))
            k += 1
        ct, acc = g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
        low = g.alloc(n * 2 * (L - 1) * N)
        g.fill_uniform(ct, n * 2 * L, list(range(L)), 3)
        ks = g.rotate_sum(L, n, ct, steps, acc)
        t_top = timed(g, lambda: g.rotate_sum(L, n, ct, steps, acc), 2)
        report(f"rotate_sum {len(steps)} steps ({ks} key switches) at L = {L}", n, t_top)

        def switched():
            g.bfv_mod_switch(L, L - 1, 2, n, ct, low)
            g.rotate_sum(L - 1, n, low, steps, acc)
        t_low = timed(g, switched, 2)
        report(f"bfv_mod_switch {L} -> {L - 1} + rotate_sum at L = {L - 1}", n, t_low, None, f"  ratio to L = {L}: {t_low[1] / t_top[1]:.3f}")
    g.close()
