#!/usr/bin/env python3
"""A PIR database from packed bytes to NTT-form plaintexts on the device, for N = 8192 {60,40,60} (L_top = 2) and N = 32768 {60,40,40,60}
(L_top = 3), n in {1024, 16384} plaintexts of B = Bmax bytes each, contiguous (stride = B), L_out = L_top.
* (a) he355_bfv_unpack_bytes_ntt (the fields are cut and lifted inside the forward column pass) against (b) he355_bfv_unpack_bytes +
  he355_bfv_plain_to_ntt, the definition and the yardstick.  The two alternate inside one process (a, b, a, b, ...), every region is
  HIP-event timed on the context's stream (he355_timer_begin / _end), every shape is warmed up first, and the figures are min / median / max
  over the regions.  (a) and (b) are compared bit for bit (the whole slab) before anything is timed.  Acceptance: (a)'s median is below
  (b)'s by more than the spread (max - min) of (b)'s own regions; a shape that misses it belongs on (b).
* (c) what a caller had before: he355_upload of the widened [n][N] 64-bit slab + he355_bfv_plain_to_ntt, against he355_upload of the bytes +
  (a); the bus time (the uploads alone, from ordinary host memory) is reported separately from the device time.
* (d) streaming rate of he355_bfv_unpack_bytes and he355_bfv_pack_bytes in compulsory bytes (every input byte read once, every output
  byte written once) per second, beside he355_add (k_addsub) over slabs of the same size in the same run.
The report goes to stdout and to profiles/bfv_database.txt.
Usage: python tools/bfv_database_probe.py [regions] [calls per region] [n ...]"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.probe_common import At, alternated, fmt

be = importlib.import_module("reference-seal-backend_amd")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
NS = [int(a) for a in sys.argv[3:]] or [1024, 16384]
RINGS = ((8192, [60, 40, 60]), (32768, [60, 40, 40, 60]))
report = open(os.path.join(ROOT, "profiles", "bfv_database.txt"), "w")


def say(line=""):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


def shape(g, N, n):
    L_out = g.L
    B, w = g.bfv_bytes_per_plain()
    host_bytes = np.random.default_rng(n).integers(0, 2 ** 64, n * B // 8, dtype=np.uint64)  # (B = N w / 8 is a multiple of 8 here)
    src, plain = g.alloc(n * B // 8), g.alloc(n * N)
    out, ref = g.alloc(n * L_out * N), g.alloc(n * L_out * N)
    src.upload(host_bytes)

    def fused(dst=out):
        g.bfv_unpack_bytes_ntt(L_out, n, src, 0, B, B, dst)

    def composed(dst=ref):
        g.bfv_unpack_bytes(n, src, 0, B, B, plain)
        g.bfv_plain_to_ntt(L_out, n, plain, dst)

    fused()
    composed()
    step = 256 * L_out * N  # compared in pieces: the whole slab, without a host copy of all of it at once
    for off in range(0, n * L_out * N, step):
        k = min(step, n * L_out * N - off)
        if not np.array_equal(out.download_range(off, (k,)), ref.download_range(off, (k,))):
            raise SystemExit(f"N {N} n {n}: he355_bfv_unpack_bytes_ntt and the composition differ")
    ta, tb = alternated(g, [fused, composed], [calls, calls], repeats, warmup=1)
    spread = tb[2] - tb[0]
    verdict = "accepted" if ta[1] < tb[1] - spread else "NOT accepted: not faster than the composition by more than its spread"
    written = n * L_out * N * 8
    say(f"N = {N} L_out = {L_out}  n {n}  B = {B} bytes (w = {w})   us per call, min / median / max of {repeats} regions")
    say(f"  (a) he355_bfv_unpack_bytes_ntt                      {fmt(ta)}   {written / ta[1] / 1e6:6.3f} TB/s of output written"
        f" ({(n * B + 3 * written) / ta[1] / 1e6:6.3f} TB/s with the row pass's read and write)")
    say(f"  (b) he355_bfv_unpack_bytes + he355_bfv_plain_to_ntt {fmt(tb)}   (b) / (a) {tb[1] / ta[1]:6.3f}   spread of (b) {spread:9.1f} us"
        f" ({spread / tb[1] * 100:4.1f} %)   {verdict}")
    # (c) the path a caller had before: the widened slab over the bus, then the transform
    wide = plain.download()
    pt = lambda: g.bfv_plain_to_ntt(L_out, n, plain, ref)
    tw, tn, tp, tf = alternated(g, [lambda: plain.upload(wide), lambda: src.upload(host_bytes), pt, fused], [1, 1, calls, calls], repeats, warmup=1)
    say(f"  (c) before: upload of the widened slab ({wide.nbytes} bytes) {fmt(tw)}  + he355_bfv_plain_to_ntt {fmt(tp)}   median sum {tw[1] + tp[1]:11.1f}")
    say(f"      now   : upload of the bytes        ({host_bytes.nbytes} bytes) {fmt(tn)}  + (a)                    {fmt(tf)}   median sum {tn[1] + tf[1]:11.1f}"
        f"   before / now {(tw[1] + tp[1]) / (tn[1] + tf[1]):6.3f} (bus alone {tw[1] / tn[1]:6.3f}, device alone {tp[1] / tf[1]:6.3f})")
    del wide
    # (d) streaming rates
    back = g.alloc(n * B // 8)
    g.bfv_pack_bytes(n, plain, B, B, back)
    if not np.array_equal(back.download(), host_bytes):
        raise SystemExit(f"N {N} n {n}: pack(unpack(x)) != x")
    m = n // 2  # he355_add over [m][2][1][N]: three slabs of n N words
    fs = [lambda: g.bfv_unpack_bytes(n, src, 0, B, B, plain), lambda: g.bfv_pack_bytes(n, plain, B, B, back),
          lambda: g.add(1, 2, m, out, At(out, n * N), be.Context.pairwise(), ref)]
    ts = alternated(g, fs, [calls] * 3, repeats, warmup=1)
    for name, t, nbytes in (("he355_bfv_unpack_bytes", ts[0], n * B + n * N * 8), ("he355_bfv_pack_bytes  ", ts[1], n * B + n * N * 8),
                            ("he355_add (k_addsub)  ", ts[2], 3 * n * N * 8)):
        say(f"  (d) {name} {nbytes:13d} compulsory bytes: {fmt(t)} us -> {nbytes / t[1] / 1e6:6.3f} TB/s at the median")
    for b in (src, plain, out, ref, back):
        b.free()
    g.pool_trim()


for N, bits in RINGS:
    g = be.Context(be.SCHEME_BFV, N, bit_sizes=bits, plain_bits=20, sec128=False, device=0)
    say(f"== N = {N} {bits}  L_top = {g.L}  t = {g.t}  (Bmax, w) = {g.bfv_bytes_per_plain()}")
    for n in NS:
        shape(g, N, n)
    g.close()
report.close()
