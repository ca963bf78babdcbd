"""Regenerates tests/golden/explicit_moduli.json: chains of moduli the prime-size rule never makes (tests/explicit_moduli.py says why).

Primes come from sympy (independent of the oracle and of the product).  No threshold is written down here: each is found by bisecting
the library's own host functions -- ff_direct_terms / ff_x_bound of tests/floor_forms_host.cpp, compiled here with the host compiler --
or the class rule restated in tests/explicit_moduli.py, and the nearest NTT-friendly primes on each side are taken.

    python tests/golden/make_explicit_moduli.py        # rewrites the JSON

tests/test_explicit_moduli_cpu.py calls build_doc() and compares where sympy is present."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import sympy

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import explicit_moduli as xm  # noqa: E402

CSRC = os.path.join(TESTS, "..", "reference-seal-backend_amd", "csrc")


def host_lib(directory):
    so = os.path.join(directory, "libfloor_forms_gen.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DHE355_U64_FOLD=0", "-I", CSRC,
                    os.path.join(TESTS, "floor_forms_host.cpp"), os.path.join(CSRC, "he_params.cpp"), "-o", so], check=True)
    S = C.CDLL(so)
    S.ff_direct_terms.restype = C.c_uint32
    S.ff_direct_terms.argtypes = [C.c_uint64]
    S.ff_x_bound.restype = C.c_double
    S.ff_x_bound.argtypes = [C.c_uint64]
    S.ff_x_max.restype = C.c_double
    return S


def up(N, lo, count=1):
    """the `count` smallest primes 1 (mod 2N) that are >= lo, ascending"""
    v = (lo - 1 + 2 * N - 1) // (2 * N) * (2 * N) + 1
    out = []
    while len(out) < count:
        if sympy.isprime(v):
            out.append(v)
        v += 2 * N
    return out


def down(N, hi, count=1):
    """the `count` largest primes 1 (mod 2N) below hi, descending"""
    v = (hi - 2) // (2 * N) * (2 * N) + 1
    out = []
    while len(out) < count:
        assert v > 2 * N
        if sympy.isprime(v):
            out.append(v)
        v -= 2 * N
    return out


def big_c(N, count):
    """the primes 2^60 - c with the largest c the fold form admits"""
    ps = up(N, (1 << 60) - xm.FOLD_MAX_C + 1, count)
    assert all(xm.fold_prime_ok(p) and xm.fold_c(p).bit_length() == 26 for p in ps)
    return ps


def batching_t(N):
    return down(N, 1 << 32)[0]


def prime_with_run(N, run):
    """the largest prime whose 128-bit sums take exactly `run` terms: its last full sum sits right under 2^128"""
    lo, hi = 1 << 59, (1 << 60) - 1
    top = xm.bisect_last_true(lambda q: xm.mac_run(q) >= run, lo, hi)
    q = down(N, top + 1)[0]
    assert xm.mac_run(q) == run
    return q


def chains_for(N, small):
    """the chains every ring gets (small: the N = 1024 variants, which keep only what the integer model runs)"""
    r60 = down(N, 1 << 60, 2)
    big = big_c(N, 2)
    f45, f40, u50 = down(N, 1 << 45)[0], down(N, 1 << 40)[0], down(N, 1 << 50)[0]
    low60 = up(N, (1 << 59) + 1)[0]
    out = []

    def add(cid, primes, t, why, **extra):
        assert len(set(primes)) == len(primes)
        e = {"id": cid + ("_n1024" if small else ""), "N": N, "primes": [hex(p) for p in primes], "t": t, "for": why}
        e.update(extra)
        out.append(e)

    add("fold_c_ends_mixed", [big[0], f45, r60[0], big[1]], 0, "both ends of c in one chain, an fp64 target between")
    add("shoup_by_one_low60", [r60[0], r60[1], low60, big[0]], 0, "one 60-bit prime from the bottom of its binade selects the Shoup form")
    e47 = up(N, (1 << 47) + 1, 2)
    add("engine_edge_47", [e47[0], down(N, 1 << 47)[0], up(N, (1 << 46) + 1)[0], e47[1]], 0,
        "the smallest u64-engine primes beside the largest and the smallest 47-bit fp64 primes")
    add("tiny", [r60[0], 12289, 40961, up(N, (1 << 30) + 1)[0], big[0]], 0, "14- to 31-bit fp64 primes under 60-bit digits, a fold special prime")
    add("unsorted_small_special", [f40, u50, r60[0], down(N, 1 << 30)[0]], 0, "the special prime is the chain's smallest: P far below every data prime")
    # the BFV twins
    a46 = down(N, 1 << xm.AUX_BITS, 2)
    q337 = prime_with_run(N, 337)
    tb = batching_t(N)
    twins = {
        "fold_c_ends_mixed": ([big[0], f45, r60[0], big[1]], [2, 1 << 31, 3 * 12289]),
        "tiny": ([r60[0], 12289, 40961, up(N, (1 << 30) + 1)[0], big[0]], [(1 << 32) - 5, tb, 256]),
        "aux46": ([a46[0], a46[1], r60[0]], [256, tb]),
        "shoup_by_one_low60": ([r60[0], r60[1], low60, big[0]], [2, 256, (1 << 32) - 5, 1 << 31]),
        "mac_337": ([q337, f40, r60[0]], [1 << 16, tb, 3 * 12289]),
    }
    why = {
        "fold_c_ends_mixed": "the fold form at both ends of c under BFV",
        "tiny": "BFV over 14- to 31-bit primes",
        "aux46": "the chain holds the first primes of the device's auxiliary base: the base must leave them out",
        "shoup_by_one_low60": "the Shoup form by one prime; its 128-bit sums take 1023 terms",
        "mac_337": "prime 0 takes 337-term sums, the last full one right under 2^128",
    }
    for cid, (primes, ts) in twins.items():
        for t in ts:
            add(f"{cid}_t{t}", primes, t, why[cid], chain=cid, batching=(t - 1) % (2 * N) == 0 and bool(sympy.isprime(t)))
    return out


def build_doc(directory=None):
    with tempfile.TemporaryDirectory() as tmp:
        S = host_lib(directory or tmp)
        doc = {"chains": []}

        def add(cid, N, primes, why, **extra):
            assert len(set(primes)) == len(primes)
            e = {"id": cid, "N": N, "primes": [hex(p) for p in primes], "t": 0, "for": why}
            e.update(extra)
            doc["chains"].append(e)

        add("fold_max_c_x7", 4096, big_c(4096, 7), "full runs of the key product at the largest c")
        add("fold_max_c_n32768", 32768, big_c(32768, 3), "the five-stage column pass at the largest c")
        N = 2048
        doc["chains"] += chains_for(N, False)
        r60 = down(N, 1 << 60, 2)
        # q_j on either side of 2 q_t: direct, and the re-centring lift
        qt = down(N, 1 << 45)[0]
        add("ratio_two", N, [qt, down(N, 2 * qt)[0], up(N, 2 * qt + 1)[0], r60[0]], "direct and re-centring lift: the nearest primes on either side of 2 q_t, 2^-26 of q_j apart")
        # the 48-bit rows' threshold, per ring: the digit of a 60-bit prime enters the column pass below q_t
        for n in (2048, 4096, 32768):
            logn1 = n.bit_length() - 11
            edge = xm.bisect_last_true(lambda q: xm.fits48_wide(q, logn1), 1 << 45, (1 << 47) - 1)
            w60 = down(n, 1 << 60, 2)
            q_in, q_out = down(n, edge + 1)[0], up(n, edge + 1)[0]
            add(f"fits48_inside_{n}", n, [w60[0], q_in, down(n, q_in)[0], w60[1]], "the fullest 48-bit rows the class rule admits", target=1, digit=2)
            add(f"fits48_outside_{n}", n, [w60[0], q_out, up(n, q_out + 1)[0], w60[1]], "the general path right beside them", target=1, digit=2)
        # the x-bound of the direct floor forms: acc_terms = (L + 3 at some L) just inside, 0 just outside
        edge = xm.bisect_last_true(lambda q: S.ff_direct_terms(q) > 0, 1 << 44, 1 << 46)
        assert S.ff_x_bound(edge) <= S.ff_x_max() < S.ff_x_bound(edge + 1)
        acc = S.ff_direct_terms(down(N, edge + 1)[0])
        n_f64 = acc - xm.TENSOR_TERMS  # the level whose c1 sums hold exactly acc terms
        inside, outside = down(N, edge + 1, n_f64), up(N, edge + 1, n_f64)
        assert all(S.ff_direct_terms(q) == acc for q in inside) and not any(S.ff_direct_terms(q) for q in outside)
        add("xbound_inside", N, [r60[0]] + inside + [r60[1]], "terms == acc_terms one level below the top, acc_terms + 1 at the top", acc_terms=acc)
        add("xbound_outside", N, [r60[0]] + outside + [r60[1]], "acc_terms == 0: every launch re-centres first", acc_terms=0)
        doc["chains"] += chains_for(1024, True)
    return doc


def main():
    with open(os.path.join(HERE, "explicit_moduli.json"), "w") as f:
        json.dump(build_doc(), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
