#!/usr/bin/env python3
"""Generates tests/golden/ckks_complex_vectors.json: what the complex CKKS codec needs beyond client_edge_vectors.json, computed with mpmath
at several hundred bits (the transforms of make_client_edge_vectors.py) -- no product code; the oracle is used only to be measured against
the exact values.

encode  N in {1024, 4096}, chain {60,45,45,60}, scale 2^40, counts 1, N/2 - 1 and N/2 of tests/ckks_complex_operands.complex_input (both
        parts uniform in [-0.7, 0.7]: inside the unit disc): the exact real coefficients of the polynomial with z[slot] = v and
        z[conjugate slot] = conj(v); kept: round(c_n * 2^16) at 16 sampled positions and E_np, the largest |coefficient of the oracle's
        numpy encoder - c_n| over ALL n.
decode  the operands of client_edge_vectors.json's decode cases on {60 x 5} at N = 2048, L = 4 and on {60, 45 x 15, 60} at N = 1024 for
        L = 1, 8 and 16: the exact IMAGINARY parts of the slots (that file holds the real parts); kept: the correctly rounded doubles at
        its slot positions and E_np_im, the largest |imaginary part of the oracle's numpy decoder - exact| over ALL slots.
Usage: python tests/golden/make_ckks_complex_vectors.py   (under a minute; writes the same bytes every time)."""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ckks_complex_operands as cx  # noqa: E402
import client_operands as co  # noqa: E402
import oracle as ho  # noqa: E402
from make_client_edge_vectors import dft, positions, roots  # noqa: E402

OUT = os.path.join(HERE, "ckks_complex_vectors.json")


def encode_exact(values, N, scale, w, twist):
    e = ho._slot_exponents(N)
    z = [mp.mpc(0)] * N
    for i, v in enumerate(values):
        z[(int(e[i]) - 1) // 2] = mp.mpc(mp.mpf(float(v.real)), mp.mpf(float(v.imag)))
        z[(2 * N - int(e[i]) - 1) // 2] = mp.mpc(mp.mpf(float(v.real)), -mp.mpf(float(v.imag)))
    f = dft(z, w)
    s = mp.mpf(scale) / N
    return [(f[n] * twist[n]).real * s for n in range(N)]


def main():
    old = co.load_fixture()
    doc = {"about": "see make_ckks_complex_vectors.py", "positions": {}, "encode": [], "decode": []}
    mp.mp.prec = 320
    for N in co.CKKS_ENCODE_N:
        o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=co.CKKS_ENCODE_CHAIN, sec128=False)
        w = roots(N, -1)
        twist = [mp.mpc(mp.cospi(mp.mpf(n) / N), -mp.sinpi(mp.mpf(n) / N)) for n in range(N)]
        pos = positions(N, 16, "cplx")
        doc["positions"][str(N)] = pos
        for count in cx.counts(N):
            values = cx.complex_input(N, count)
            exact = encode_exact(values, N, cx.SCALE, w, twist)
            got = co.coeffs_from_plain(o, ho.ckks_encode(o, values, cx.SCALE))
            e_np = max(abs(mp.mpf(g) - c) for g, c in zip(got, exact))
            doc["encode"].append({"id": f"N{N}/count{count}", "N": N, "count": count, "digest": co.digest(values.view(np.float64)), "E_np": float(e_np).hex(),
                                  "exact_x65536": [str(int(mp.nint(exact[p] * 65536))) for p in pos]})
            print(doc["encode"][-1]["id"], "E_np", float(e_np), flush=True)
    mp.mp.prec = 1400
    for chain, levels in cx.DECODE_LEVELS.items():
        N, bits, _ = co.DECODE_CHAINS[chain]
        o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
        w = roots(N, +1)
        twist = [mp.mpc(mp.cospi(mp.mpf(n) / N), mp.sinpi(mp.mpf(n) / N)) for n in range(N)]
        e = ho._slot_exponents(N)
        for L in levels:
            mods = [int(q) for q in o.moduli[:L]]
            Q = co.prod(mods)
            for fam in co.DECODE_FAMILIES:
                coeffs = co.decode_coefficients(fam, Q, N)
                res = co.to_residues(coeffs, mods)
                plain = np.stack([o.ntt(i, res[i]) for i in range(L)])
                f = dft([mp.mpf(c) * twist[n] for n, c in enumerate(coeffs)], w)
                unit = [f[(int(x) - 1) // 2].imag for x in e[:N // 2]]
                for sname in co.DECODE_SCALES[fam]:
                    scale = co.decode_scale(sname, Q)
                    exact = [v / mp.mpf(scale) for v in unit]
                    got = ho.ckks_decode(o, plain, scale).imag
                    e_np = max(abs(mp.mpf(float(g)) - v) for g, v in zip(got, exact))
                    doc["decode"].append({"id": f"{chain}/L{L}/{fam}/{sname}", "digest": co.digest(coeffs), "E_np_im": float(e_np).hex(),
                                          "exact_im": [float(exact[p]).hex() for p in old["slot_positions"][str(N)]]})
                    print(doc["decode"][-1]["id"], "E_np_im", float(e_np), flush=True)
    with open(OUT, "w") as fh:
        fh.write('{"about":' + json.dumps(doc["about"]) + ',\n"positions":' + json.dumps(doc["positions"], separators=(",", ":")))
        for key in ("encode", "decode"):
            fh.write(',\n"' + key + '":[\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in doc[key]) + "\n]")
        fh.write("}\n")
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
