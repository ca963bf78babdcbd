"""The layouts the hoisted rotation family is held to beyond the table of tests/test_gpu_rotate_hoisted.py (a plain helper module, no device
and no test in it: tests/test_hoisted_layouts_ref_cpu.py and tests/test_gpu_hoisted_layouts.py import it).

An entry gives the scheme, N, the chain -- by bit sizes under the prime-size rule (sec128 off) or by the id of a chain of
tests/golden/explicit_moduli.json -- the plain modulus (BFV by bits: plain_bits 20; from the fixture: its t) and what the layout is for:
the path of csrc/he355_kernels_hoist.hip that no context of the older table reaches.

    hoist_sp_row<ArF64>    the special prime in the fp64 engine (P < 2^47): the raw words made canonical, the forward row pass, 1024^-1 taken
                           out; `last` (N = 1024: the row pass is the whole transform, fix = 1); logn1 = 2 and 5; under BFV
    large rings            N = 16384 and 32768 through the lazy sum and the transform: the source row, rowbase = n1 + srow, the twiddle slice
                           and the permutation tables at their largest
    moduli                 the chains of the fixture: P far below the data primes (hoist_centred_mod, bsgs_p_mod / bsgs_fold_c0), barrett64 of
                           a 60-bit P under a 14-bit modulus, the engine edge at 2^47, fold primes at the largest c, the Shoup form selected
                           by one prime (k_key_permute moves the per-element quotient blocks)
    levels                 K = 5: hoist_qp_prime jumps from tile L to prime K - 1 across unused primes; L = 1 reads one of the key's digits"""
from __future__ import annotations

import explicit_moduli as xm
import shoup_rings as sr

PLAIN_BITS = 20
_FIXTURE = None


def _ckks(N, bits, form, what):
    return {"scheme": "ckks", "N": N, "bits": bits, "fixture": None, "plain_bits": 0, "form": form, "for": what}


def _bfv(N, bits, form, what):
    return {"scheme": "bfv", "N": N, "bits": bits, "fixture": None, "plain_bits": PLAIN_BITS, "form": form, "for": what}


def _fix(scheme, cid, form, what):
    return {"scheme": scheme, "N": None, "bits": None, "fixture": cid, "plain_bits": 0, "form": form, "for": what}


LAYOUTS = {
    # CKKS by bit sizes
    "f64_only_1024": _ckks(1024, [42, 38, 44], None, "hoist_sp_row<ArF64>, the `last` branch: the row pass is the whole transform, fix = 1"),
    "f64_only_4096": _ckks(4096, [46, 40, 40, 46], None, "hoist_sp_row<ArF64> at logn1 = 2"),
    "f64_only_32768": _ckks(32768, [46, 40, 46], None, "hoist_sp_row<ArF64> at logn1 = 5"),
    "n16384": _ckks(16384, [60, 45, 60], "fold", "the lazy sum and the transform above N = 8192"),
    "n32768": _ckks(32768, [60, 45, 60], "fold", "the largest ring, default engines"),
    "deep_4096": _ckks(4096, [60, 40, 40, 40, 60], "fold", "L = 1 and 2 under K = 5: tile L is prime K - 1 across unused primes; one key digit of four"),
    # the chains of tests/shoup_rings.py: the Shoup build of the u64 engine above N = 8192, a 60- and a 50-bit prime on it
    "n8192_shoup": _ckks(8192, list(sr.MIXED), "shoup", "the Shoup form at logn1 = 3"),
    "n16384_shoup": _ckks(16384, list(sr.MIXED), "shoup", "the Shoup form at logn1 = 4: the lazy sum, the transform and k_key_permute's quotient blocks"),
    "n32768_shoup": _ckks(32768, list(sr.MIXED), "shoup", "the Shoup form on the largest ring"),
    # CKKS from the fixture
    "tiny": _fix("ckks", "tiny", "fold", "a 60-bit P and 59-bit centred coefficients under 14- to 31-bit moduli"),
    "tiny_n1024": _fix("ckks", "tiny_n1024", "fold", "the same with one row per polynomial"),
    "unsorted_small_special": _fix("ckks", "unsorted_small_special", "shoup", "P of 30 bits far below the data primes, in the fp64 engine under u64 data primes"),
    "unsorted_small_special_n1024": _fix("ckks", "unsorted_small_special_n1024", "shoup", "the same through the `last` branch"),
    "engine_edge_47": _fix("ckks", "engine_edge_47", "shoup", "both engines at their edge, 2^47"),
    "shoup_by_one_low60": _fix("ckks", "shoup_by_one_low60", "shoup", "the Shoup form by one prime: k_key_permute moves the quotient blocks of 60-bit primes"),
    "shoup_by_one_low60_n1024": _fix("ckks", "shoup_by_one_low60_n1024", "shoup", "the same with one row per polynomial"),
    "fold_c_ends_mixed": _fix("ckks", "fold_c_ends_mixed", "fold", "fold primes at both ends of c, an fp64 prime between"),
    "fold_max_c_x7": _fix("ckks", "fold_max_c_x7", "fold", "seven fold primes at the largest c"),
    "fold_max_c_n32768": _fix("ckks", "fold_max_c_n32768", "fold", "fold primes at the largest c on the largest ring"),
    # BFV: the eager call in both forms, the lazy sum and the transform on NTT-form residues
    "bfv_f64_only_1024": _bfv(1024, [42, 38, 44], None, "hoist_sp_row<ArF64> under BFV, `last`"),
    "bfv_f64_only_4096": _bfv(4096, [42, 38, 45, 44], None, "hoist_sp_row<ArF64> under BFV, logn1 = 2, three data primes"),
    "bfv_n16384_shoup": _bfv(16384, list(sr.MIXED), "shoup", "the Shoup form at logn1 = 4 under BFV: the eager call in both forms"),
    "bfv_tiny_t256": _fix("bfv", "tiny_t256", "fold", "BFV over 14- to 31-bit primes"),
    "bfv_aux46_t256": _fix("bfv", "aux46_t256", "fold", "fp64 data primes of the auxiliary base's size under a 60-bit P"),
    "bfv_mac_337_t65536": _fix("bfv", "mac_337_t65536", "shoup", "a prime whose 128-bit sums take 337 terms beside a 256-term one"),
    "bfv_shoup_by_one_low60_t256": _fix("bfv", "shoup_by_one_low60_t256", "shoup", "the Shoup form by one prime under BFV"),
    "bfv_fold_c_ends_mixed_t2": _fix("bfv", "fold_c_ends_mixed_t2", "fold", "the fold form at both ends of c under BFV, t = 2"),
}
CKKS = [k for k, e in LAYOUTS.items() if e["scheme"] == "ckks"]
BFV = [k for k, e in LAYOUTS.items() if e["scheme"] == "bfv"]
# the layouts whose lazy sum and transform also run with every operand and the key at q - 1, and then with c1 = 0
EDGED = [k for k in LAYOUTS if k.startswith(("f64_only_", "tiny", "unsorted_small_special")) or k == "fold_max_c_x7"]
STEPS = (1, 3, -2)


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        _FIXTURE = xm.load()
    return _FIXTURE


def entry(name):
    """the entry with N, primes (None: by bit sizes) and t (0: CKKS; None: plain_bits) filled in from the fixture"""
    e = dict(LAYOUTS[name])
    e["primes"], e["t"] = None, 0 if e["scheme"] == "ckks" else None
    if e["fixture"]:
        c = fixture()[e["fixture"]]
        assert bool(c["t"]) == (e["scheme"] == "bfv"), name
        e["N"], e["primes"], e["t"], e["bits"] = c["N"], list(c["primes"]), c["t"], xm.bits_of(c["primes"])
    return e


def make_oracle(oracle, name):
    e = entry(name)
    if e["primes"] is not None:
        scheme = oracle.SCHEME_CKKS if e["scheme"] == "ckks" else oracle.SCHEME_BFV
        o = oracle.Context(scheme, e["N"], primes=e["primes"], plain_modulus=e["t"])
    elif e["scheme"] == "ckks":
        o = oracle.Context(oracle.SCHEME_CKKS, e["N"], bit_sizes=e["bits"], sec128=False)
    else:
        o = oracle.Context(oracle.SCHEME_BFV, e["N"], bit_sizes=e["bits"], plain_bits=e["plain_bits"], sec128=False)
    check_chain(name, o.moduli)
    return o


def check_chain(name, moduli):
    """the chain a context made is the table's: the fixture's primes themselves, or primes of the table's bit sizes"""
    e = entry(name)
    if e["primes"] is not None:
        assert list(moduli) == e["primes"], (name, "the context does not hold the fixture's chain")
    else:
        assert xm.bits_of(moduli) == e["bits"], (name, xm.bits_of(moduli))
    assert xm.form_of(moduli) == e["form"], (name, "the form of the u64 engine", xm.form_of(moduli))


def engines(moduli):
    """(fp64 flags, form) of a chain: explicit_moduli.is_f64 per prime -- what the device's he355_prime_uses_fp64 must report -- and
    explicit_moduli.form_of over the chain (the library picks the build of the u64 engine by it; it has no query for it)"""
    return [xm.is_f64(q) for q in moduli], xm.form_of(moduli)


def levels(name, L_top):
    """L_top and L = 1; deep_4096: L = 2 as well"""
    ls = [L_top] + ([1] if L_top > 1 else [])
    if name == "deep_4096":
        ls.insert(1, 2)
    return ls


def closed_form_elts(N):
    """the six elements of the c1 = 0 closed form: N + 1, N - 1, 3, 2N - 3, 5^(N/4) and 2N - 1"""
    return [N + 1, N - 1, 3, 2 * N - 3, pow(5, N // 4, 2 * N), 2 * N - 1]
