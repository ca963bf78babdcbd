#!/usr/bin/env python3
"""Seeded BFV queries and Galois keys on the device, for N = 8192 {60,40,60} and N = 32768 {60,40,40,60}, at L = L_top:
1. he355_bfv_seeded_restore(ntt_form 0) of n queries against he355_upload of the n L N words the seed saves (what the server would do with
   the second half had it travelled): both between host clock reads with a he355_sync before each read, since the upload is a host call;
2. he355_set_galois_key_seeded against he355_set_galois_key (the same key, the same way);
3. `kernel`: six he355_bfv_seeded_restore(ntt_form 1 -- the generation kernel writes n L N words, k_bfv_seeded_place copies as many, the forward
   transform runs on c0) and six he355_add over a slab of the same words and nothing else: the run to put under a kernel trace, one ring per
   run, whose per-kernel times give k_bfv_seeded_gen's write rate beside k_addsub's (a slab added to itself: one read, one written) as the
   streaming yardstick;
4. he355_bfv_seeded_encrypt against he355_encrypt on the client (HIP-event regions on the context's stream, he355_timer_begin / _end).
The candidates alternate inside one process, every shape is warmed up first, and the figures are min / median / max over the regions.
Before anything is timed the restored ciphertexts are decrypted and held to the plaintexts, and the two keys to one another through
he355_apply_galois.
Usage: python tools/bfv_seeded_probe.py [regions] [calls per region] [all | kernel] [8192 | 32768]"""
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as ho  # the secret and public key only: nothing timed goes through it
from tools.probe_common import alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
mode = sys.argv[3] if len(sys.argv) > 3 else "all"
ring = int(sys.argv[4]) if len(sys.argv) > 4 else 0  # 8192 or 32768: that ring alone
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
BATCH = 256
A_SEED, E_SEED = 0xA5EED, 0xE5EED


def ratio(ta, tb):
    return f"{tb[1] / ta[1]:6.3f} (from {tb[0] / ta[2]:6.3f} to {tb[2] / ta[0]:6.3f} over the regions' extremes)"


def host_alternated(g, fs, n_calls, regions, warmup=2):
    """probe_common.alternated between host clock reads: (min, median, max) us per call, a he355_sync before every read"""
    for f in fs:
        for _ in range(warmup):
            f()
    g.sync()
    t = [[] for _ in fs]
    for _ in range(regions):
        for k, f in enumerate(fs):
            t0 = time.perf_counter()
            for _ in range(n_calls):
                f()
            g.sync()
            t[k].append((time.perf_counter() - t0) / n_calls * 1e6)
    return [(min(v), statistics.median(v), max(v)) for v in t]


def kernel_run(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    L = g.L
    c0, out, other = g.alloc(BATCH * L * N), g.alloc(BATCH * 2 * L * N), g.alloc(BATCH * L * N)
    g.fill_uniform(c0, BATCH * L, list(range(L)), 7)
    for _ in range(6):
        g.bfv_seeded_restore(L, 1, BATCH, c0, A_SEED, 0, out)
        g.add(L, 1, BATCH, c0, c0, be.Context.pairwise(), other)
    g.sync()
    print(f"N = {N}: k_bfv_seeded_gen over {BATCH} queries at L = {L} writes {BATCH * L * N * 8} bytes and reads none; k_addsub (he355_add of a slab of"
          f" {BATCH} c0's to itself: one slab read, one written) moves {2 * BATCH * L * N * 8}", flush=True)
    g.close()


def run(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L, K, t = g.L, g.K, g.t
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    print(f"== N = {N} {bits}  L_top = {L}  t = {t}  batch {BATCH}", flush=True)
    print(f"  query bytes: {2 * L * N * 8} unseeded, {L * N * 8} + 8 seeded; Galois key bytes: {L * 2 * K * N * 8} unseeded, {L * K * N * 8} + 8 seeded")
    plain = np.random.default_rng(5).integers(0, t, (BATCH, N), dtype=np.uint64)
    dp = g.to_device(plain)
    c0, ct, full, dec = g.alloc(BATCH * L * N), g.alloc(BATCH * 2 * L * N), g.alloc(BATCH * 2 * L * N), g.alloc(BATCH * N)
    g.bfv_seeded_encrypt(L, BATCH, dp, A_SEED, E_SEED, 0, c0)
    g.bfv_seeded_restore(L, 0, BATCH, c0, A_SEED, 0, ct)
    g.decrypt(L, 2, BATCH, ct, dec)
    if not np.array_equal(dec.download((BATCH, N)), plain):
        raise SystemExit("a restored seeded ciphertext does not decrypt to its plaintext")
    budget = g.bfv_noise_budget(L, 2, BATCH, ct)
    g.encrypt(BATCH, dp, 12, 0, full)
    budget_pk = g.bfv_noise_budget(L, 2, BATCH, full)
    half = np.ascontiguousarray(ct.download((BATCH, 2, L, N))[:, 1])  # the half the seed saves, as it would have travelled
    land = g.alloc(BATCH * L * N)

    # 2. the keys
    elt = N // 2 + 1
    kb = g.alloc(L * K * N)
    g.keygen_galois_seeded(elt, A_SEED, E_SEED, kb)
    b = kb.download((L, K, N))
    g.set_galois_key_seeded(elt, b, A_SEED)
    x, y1, y2 = g.alloc(2 * L * N), g.alloc(2 * L * N), g.alloc(2 * L * N)
    g.fill_uniform(x, 2 * L, list(range(L)), 9)
    g.apply_galois(L, 1, x, elt, y1)
    # the unseeded install is timed with uniform residues (below every prime of the chain) of a full key's size: an upload and
    # key_finish, neither of which depends on what the key holds.  The seeded install is checked against itself through he355_apply_galois
    fullkey = np.random.default_rng(6).integers(0, 1 << 35, (L, 2, K, N), dtype=np.uint64)
    g.set_galois_key_seeded(elt, b, A_SEED)
    g.apply_galois(L, 1, x, elt, y2)
    if not np.array_equal(y1.download(), y2.download()):
        raise SystemExit("two installs of one seeded key disagree")

    def restore():
        g.bfv_seeded_restore(L, 0, BATCH, c0, A_SEED, 0, ct)

    def upload():
        land.upload(half)

    def set_seeded():
        g.set_galois_key_seeded(elt, b, A_SEED)

    def set_full():
        g.set_galois_key(elt, fullkey)

    def seeded_encrypt():
        g.bfv_seeded_encrypt(L, BATCH, dp, A_SEED, E_SEED, 0, c0)

    def encrypt():
        g.encrypt(BATCH, dp, 12, 0, full)

    tr, tu, ts, tf = host_alternated(g, [restore, upload, set_seeded, set_full], calls, repeats)
    g.set_galois_key_seeded(elt, b, A_SEED)
    te, tp = alternated(g, [seeded_encrypt, encrypt], [calls] * 2, repeats)
    print(f"  us per call, min / median / max of {repeats} regions of {calls} calls")
    print(f"  1. he355_bfv_seeded_restore(0) of {BATCH} queries        {fmt(tr)}   (host clock)")
    print(f"     he355_upload of the {BATCH * L * N * 8} bytes it saves       {fmt(tu)}   upload / restore {ratio(tr, tu)}")
    print(f"  2. he355_set_galois_key_seeded                     {fmt(ts)}   (host clock)")
    print(f"     he355_set_galois_key                            {fmt(tf)}   full / seeded {ratio(ts, tf)}")
    print(f"  4. he355_bfv_seeded_encrypt of {BATCH} plaintexts       {fmt(te)}   (stream events)")
    print(f"     he355_encrypt of the same                       {fmt(tp)}   public-key / seeded {ratio(te, tp)}")
    print(f"  noise budget at L = {L}: seeded {budget.min()}..{budget.max()} bits, public-key {budget_pk.min()}..{budget_pk.max()}", flush=True)
    g.close()


for N, bits in RINGS:
    if ring in (0, N):
        (kernel_run if mode == "kernel" else run)(N, bits)
