#!/usr/bin/env python3
"""BFV reply compression on the device, for N = 8192 {60,40,60} and N = 32768 {60,40,40,60}, a batch of 1024 replies, the safe widths
(bitlen(t) + 2, bitlen(t) + 2 + log2 N):
* he355_bfv_reply_compress at L = 1, and at L = L_top against he355_bfv_mod_switch(L_top -> 1) + the L = 1 call (the same two launches);
* he355_bfv_reply_decrypt against he355_decrypt of the uncompressed L = 1 replies (one transform fewer per reply), the ratio with the spread;
* the reply bytes before and after;
* the budget he355_bfv_reply_decrypt reports at the safe widths and at k1 lowered step by step (k0 = min(k0, k1)) until the first wrong
  coefficient (64 replies): what a user needs to pick tighter widths -- an observation on these keys and these fresh replies, not a guarantee.
The candidates alternate inside one process, every region is HIP-event timed on the context's stream (he355_timer_begin / _end), every
shape is warmed up first, and the figures are min / median / max over the regions.  The replies are fresh encryptions of full-range
plaintexts (keys: the oracle's) switched to L = 1; before anything is timed the decrypted replies are held to he355_decrypt.
`kernel`: six he355_bfv_reply_compress calls at L = 1 and six he355_add over slabs of the same batch (uniform residues, no keys) and nothing
else: the run to put under a kernel trace, one ring per run, whose per-kernel times give k_bfv_reply_pack's rate in compulsory bytes
(2 N 8 read, N (k0 + k1) / 8 written per reply) beside k_addsub's (a slab added to itself: one read, one written) as the streaming yardstick.
Usage: python tools/bfv_reply_probe.py [regions] [calls per region] [all | kernel] [8192 | 32768]"""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oracle as ho  # keys only: nothing timed goes through it
from tools.probe_common import At, alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 4
mode = sys.argv[3] if len(sys.argv) > 3 else "all"
ring = int(sys.argv[4]) if len(sys.argv) > 4 else 0  # 8192 or 32768: that ring alone
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
BATCH = 1024
SCAN = 64  # replies of the width scan
ENC = 256  # plaintexts of one he355_encrypt call; reply i encrypts plaintext i % ENC


def ratio(ta, tb):
    return f"{tb[1] / ta[1]:6.3f} (from {tb[0] / ta[2]:6.3f} to {tb[2] / ta[0]:6.3f} over the regions' extremes)"


def kernel_run(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    k0, k1, _ = g.bfv_reply_safe_bits()
    B = g.bfv_reply_bytes(k0, k1)
    low, other, wire = g.alloc(BATCH * 2 * N), g.alloc(BATCH * 2 * N), g.alloc(BATCH * B // 8)
    g.fill_uniform(low, BATCH * 2, [0], 7)  # uniform residues mod q_0: the rate does not depend on what the replies decrypt to
    for _ in range(6):
        g.bfv_reply_compress(1, k0, k1, BATCH, low, wire, B)
        g.add(1, 2, BATCH, low, low, be.Context.pairwise(), other)
    g.sync()
    print(f"N = {N}: k_bfv_reply_pack over {BATCH} replies moves {BATCH * (2 * N * 8 + B)} compulsory bytes, k_addsub (he355_add of a slab of {BATCH} L = 1"
          f" ciphertexts to itself: one slab read, one written) {2 * BATCH * 2 * N * 8}", flush=True)
    g.close()


def run(N, bits):
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    o = ho.Context(ho.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False)
    L, t = g.L, g.t
    sk = o.keygen_secret(1)
    g.set_secret_key(sk)
    g.set_public_key(o.keygen_public(sk, 2))
    k0, k1, ok = g.bfv_reply_safe_bits()
    B = g.bfv_reply_bytes(k0, k1)
    print(f"== N = {N} {bits}  L_top = {L}  t = {t}  safe widths ({k0}, {k1}) accepted: {ok}", flush=True)
    print(f"  reply bytes: {2 * N * 8} at L = 1 uncompressed, {B} compressed ({B / (2 * N * 8) * 100:.1f} %)")
    plain = np.random.default_rng(5).integers(0, t, (ENC, N), dtype=np.uint64)
    dplain = g.to_device(plain)
    top = g.alloc(BATCH * 2 * L * N)
    for b in range(0, BATCH, ENC):
        g.encrypt(ENC, dplain, 12, b, At(top, b * 2 * L * N))
    low, low2 = g.alloc(BATCH * 2 * N), g.alloc(BATCH * 2 * N)
    g.bfv_mod_switch(L, 1, 2, BATCH, top, low)
    wire, wire2 = g.alloc(BATCH * B // 8), g.alloc(BATCH * B // 8)
    out, out2 = g.alloc(BATCH * N), g.alloc(BATCH * N)
    g.decrypt(1, 2, BATCH, low, out2)
    want = out2.download((BATCH, N))
    assert np.array_equal(want[:ENC], plain)
    budget1 = g.bfv_noise_budget(1, 2, BATCH, low)

    def compress():
        g.bfv_reply_compress(1, k0, k1, BATCH, low, wire, B)

    def compress_top():
        g.bfv_reply_compress(L, k0, k1, BATCH, top, wire2, B)

    def two_calls():
        g.bfv_mod_switch(L, 1, 2, BATCH, top, low2)
        g.bfv_reply_compress(1, k0, k1, BATCH, low2, wire2, B)

    def reply_decrypt():
        g.bfv_reply_decrypt(k0, k1, BATCH, wire, B, out)

    def decrypt():
        g.decrypt(1, 2, BATCH, low, out2)

    compress()
    compress_top()
    if not np.array_equal(wire.download(), wire2.download()):
        raise SystemExit("compress at L_top differs from mod_switch + compress at L = 1")
    budget, bits_ = g.bfv_reply_decrypt(k0, k1, BATCH, wire, B, out, with_budget=True)
    if not np.array_equal(out.download((BATCH, N)), want):
        raise SystemExit("he355_bfv_reply_decrypt at the safe widths differs from he355_decrypt")
    tc, tt, t2, td, tu = alternated(g, [compress, compress_top, two_calls, reply_decrypt, decrypt], [calls] * 5, repeats)
    print(f"  batch {BATCH}, us per call, min / median / max of {repeats} regions of {calls} calls")
    print(f"  he355_bfv_reply_compress L = 1                     {fmt(tc)}   {BATCH * (2 * N * 8 + B) / tc[1] / 1e6:6.2f} TB/s compulsory")
    print(f"  he355_bfv_reply_compress L = {L}                     {fmt(tt)}")
    print(f"  he355_bfv_mod_switch({L} -> 1) + compress at L = 1   {fmt(t2)}   two calls / one call {ratio(tt, t2)}")
    print(f"  he355_bfv_reply_decrypt                            {fmt(td)}")
    print(f"  he355_decrypt of the uncompressed L = 1 replies    {fmt(tu)}   decrypt / reply_decrypt {ratio(td, tu)}")
    print(f"  noise budget of the replies at L = 1: {budget1.min()}..{budget1.max()} bits (he355_bfv_noise_budget)")
    print(f"  widths ({k0}, {k1}): budget {budget.min()}..{budget.max()}, noise_bits {bits_.min()}..{bits_.max()}, all {BATCH} replies right")
    a, b = k0, k1
    while b > 2:
        b -= 1
        a = min(a, b)
        Bx = g.bfv_reply_bytes(a, b)
        g.bfv_reply_compress(1, a, b, SCAN, low, wire, Bx)
        bu, nb = g.bfv_reply_decrypt(a, b, SCAN, wire, Bx, out, with_budget=True)
        wrong = int((out.download_head((SCAN, N)) != want[:SCAN]).sum())
        print(f"  widths ({a}, {b}): {Bx} bytes, budget {bu.min()}..{bu.max()}, noise_bits {nb.min()}..{nb.max()}, wrong coefficients {wrong} of {SCAN * N}", flush=True)
        if wrong:
            break
    g.close()


for N, bits in RINGS:
    if ring in (0, N):
        (kernel_run if mode == "kernel" else run)(N, bits)
