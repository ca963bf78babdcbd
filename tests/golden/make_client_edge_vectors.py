#!/usr/bin/env python3
"""Generates tests/golden/client_edge_vectors.json: the CKKS encoder and decoder at the operands of tests/client_operands.py, computed
with mpmath at several hundred bits -- no product code; the oracle is used only to be measured against the exact values.

encode  N in {1024, 4096}, chain {60,45,45,60}: for every input of client_operands.CKKS_INPUTS at the scales 2^30, 2^40, 2^45 the exact
        real coefficients c_n = (scale / N) * Re(zeta^-n DFT(z)[n]).  The whole vector is computed; the file keeps round(c_n * 2^16) at
        the sampled positions `positions[N]` (the whole vectors would be 40 times the size of the largest fixture here), the largest
        |c_n|, the share of coefficients within 2^-10 of a rounding tie (all positions; asserted <= 1 %, and no sampled position may be
        one), under the tie rule (scale 2^30, |c_n| < 2^31) those positions and a digest of round(c_n) at all the others, and E_np, the largest |coefficient of the oracle's numpy encoder - c_n| over ALL n.
decode  chain {60, 45 x 15, 60} at N = 1024 for every L = 1 .. 16 and {60 x 5} at N = 2048, L = 4: for every family of
        client_operands.DECODE_FAMILIES at its scales the exact slot values; kept: the correctly rounded doubles at `slot_positions[N]`,
        the largest |slot| and E_np, the largest |slot of the oracle's numpy decoder - exact| over ALL slots.
Inputs are rebuilt by the tests from client_operands; `digest` pins them.  The transform is a recursive radix-2 splitting.
Usage: python tests/golden/make_client_edge_vectors.py   (about two minutes; writes the same bytes every time)."""
import json
import os
import random
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import client_operands as co  # noqa: E402
import oracle as ho  # noqa: E402

OUT = os.path.join(HERE, "client_edge_vectors.json")


def roots(n: int, sign: int):
    """exp(sign * 2 pi i k / n), k < n, from the first octant's sines and cosines"""
    return [mp.mpc(mp.cospi(mp.mpf(2 * k) / n), sign * mp.sinpi(mp.mpf(2 * k) / n)) for k in range(n)]


def dft(x, w, stride=1):
    """sum_j x[j] w[stride * j * n]: recursive radix-2 splitting, w the table of len(x) * stride roots"""
    n = len(x)
    if n == 1:
        return [x[0]]
    ev, od = dft(x[0::2], w, stride * 2), dft(x[1::2], w, stride * 2)
    out = [None] * n
    for k in range(n // 2):
        t = od[k] * w[k * stride]
        out[k] = ev[k] + t
        out[k + n // 2] = ev[k] - t
    return out


def positions(N: int, count: int, tag: str):
    rng = random.Random(f"pos/{tag}/{N}")
    fixed = [0, 1, N // 2 - 1, N // 2, N - 1]
    out = list(fixed)
    while len(out) < count:
        p = rng.getrandbits(N.bit_length() - 1)
        if p not in out:
            out.append(p)
    return sorted(out)


def encode_exact(values, N: int, scale: float, w, twist):
    e = ho._slot_exponents(N)
    z = [mp.mpc(0)] * N
    for i, v in enumerate(values):
        z[(int(e[i]) - 1) // 2] = mp.mpc(mp.mpf(float(v)))
        z[(2 * N - int(e[i]) - 1) // 2] = mp.mpc(mp.mpf(float(v)))  # the conjugate of a real value
    f = dft(z, w)
    s = mp.mpf(scale) / N
    return [(f[n] * twist[n]).real * s for n in range(N)]


def decode_exact(coeffs, N: int, scale: float, w, twist):
    f = dft([mp.mpf(c) * twist[n] for n, c in enumerate(coeffs)], w)
    e = ho._slot_exponents(N)
    s = mp.mpf(scale)
    return [f[(int(x) - 1) // 2].real / s for x in e]


def main():
    enc_pos = {}
    dec_pos = {N: positions(N // 2, 4, "dec") for N, _, _ in co.DECODE_CHAINS.values()}
    doc = {"about": "see make_client_edge_vectors.py", "positions": None, "slot_positions": {str(k): v for k, v in dec_pos.items()},
           "encode": [], "decode": []}
    # ---- encode ------------------------------------------------------------------------------------------------------------------
    mp.mp.prec = 320
    for N in co.CKKS_ENCODE_N:
        o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=co.CKKS_ENCODE_CHAIN, sec128=False)
        w = roots(N, -1)
        twist = [mp.mpc(mp.cospi(mp.mpf(n) / N), -mp.sinpi(mp.mpf(n) / N)) for n in range(N)]
        pending = []
        for name in co.CKKS_INPUTS:
            values = co.ckks_input(name, N)
            unit = encode_exact(values, N, 1.0, w, twist)  # (the scales are powers of two: one transform per input)
            for scale in co.CKKS_SCALES:
                exact = [c * mp.mpf(scale) for c in unit]
                got = co.coeffs_from_plain(o, ho.ckks_encode(o, values, scale))
                e_np = max(abs(mp.mpf(g) - c) for g, c in zip(got, exact))
                big = max(abs(c) for c in exact)
                frac = [c - mp.floor(c) for c in exact]
                near = [n for n in range(N) if abs(frac[n] - mp.mpf(0.5)) <= co.TIE_WINDOW]
                tie_rule = scale == 2.0 ** 30 and big < 2 ** 31
                if tie_rule:  # (change the seed of the input, never the cap)
                    assert len(near) <= co.TIE_SHARE_CAP * N, (name, N, len(near))
                pending.append(({
                    "id": f"{name}/N{N}/s{int(np.log2(scale))}", "input": name, "N": N, "scale": float(scale).hex(), "digest": co.digest(values),
                    "tie_rule": bool(tie_rule), "tie_share": round(len(near) / N, 5), "max_abs": float(big).hex(), "E_np": float(e_np).hex(),
                    "exact_x65536": None}, exact, set(near) if tie_rule else set()))
                if tie_rule:  # the whole vector: the positions left out and a digest of the correctly rounded integers everywhere else
                    pending[-1][0]["near_ties"] = near
                    pending[-1][0]["rounded_digest"] = co.digest([int(mp.nint(c)) for n, c in enumerate(exact) if n not in set(near)])
                print(pending[-1][0]["id"], "E_np", float(e_np), "max", float(big), "near ties", len(near), flush=True)
        # the sampled positions of this ring: the first seeded choice that holds no near-tie coefficient of a case under the tie rule (the
        # cap on the left-out share is 1 %, and 1 % of 16 positions is none)
        for attempt in range(64):
            pos = positions(N, 16, f"enc{attempt}")
            if not any(near & set(pos) for _, _, near in pending):
                break
        else:
            raise AssertionError("no choice of sampled positions avoids the near ties")
        enc_pos[N] = pos
        for case, exact, _ in pending:
            case["exact_x65536"] = [str(int(mp.nint(exact[p] * 65536))) for p in pos]
            doc["encode"].append(case)
    # ---- decode ------------------------------------------------------------------------------------------------------------------
    mp.mp.prec = 1400  # Q < 2^736 and 2^-30 of a unit at the small end: every sum is exact to far below a double's last bit
    for chain, (N, bits, levels) in co.DECODE_CHAINS.items():
        o = ho.Context(ho.SCHEME_CKKS, N, bit_sizes=bits, sec128=False)
        w = roots(N, +1)
        twist = [mp.mpc(mp.cospi(mp.mpf(n) / N), mp.sinpi(mp.mpf(n) / N)) for n in range(N)]
        for L in levels:
            mods = [int(q) for q in o.moduli[:L]]
            Q = co.prod(mods)
            for fam in co.DECODE_FAMILIES:
                coeffs = co.decode_coefficients(fam, Q, N)
                res = co.to_residues(coeffs, mods)
                plain = np.stack([o.ntt(i, res[i]) for i in range(L)])
                unit = None
                for sname in co.DECODE_SCALES[fam]:
                    scale = co.decode_scale(sname, Q)
                    if unit is None:
                        unit = decode_exact(coeffs, N, 1.0, w, twist)
                    exact = [v / mp.mpf(scale) for v in unit]
                    got = ho.ckks_decode(o, plain, scale).real
                    e_np = max(abs(mp.mpf(float(g)) - v) for g, v in zip(got, exact))
                    doc["decode"].append({
                        "id": f"{chain}/L{L}/{fam}/{sname}", "scale": float(scale).hex(),
                        "digest": co.digest(coeffs), "magnitude": float(max(abs(v) for v in exact)).hex(), "E_np": float(e_np).hex(),
                        "exact": [float(exact[p]).hex() for p in dec_pos[N]]})
                    print(doc["decode"][-1]["id"], "E_np", float(e_np), "magnitude", float.fromhex(doc["decode"][-1]["magnitude"]), flush=True)
    doc["positions"] = {str(k): v for k, v in enc_pos.items()}
    with open(OUT, "w") as f:
        f.write('{"about":' + json.dumps(doc["about"]) + ',\n"positions":' + json.dumps(doc["positions"], separators=(",", ":")) +
                ',\n"slot_positions":' + json.dumps(doc["slot_positions"], separators=(",", ":")))
        for key in ("encode", "decode"):
            f.write(',\n"' + key + '":[\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in doc[key]) + "\n]")
        f.write("}\n")
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(doc['encode'])} encode and {len(doc['decode'])} decode cases")


if __name__ == "__main__":
    main()
