"""The Shoup-form chains the suite runs at N >= 8192 (a plain helper module, no device and no test in it: the table-driven GPU modules,
their helper modules and tests/test_instantiation_matrix_cpu.py import it).

Every file with device code is built twice -- the fold form, for chains whose u64-engine primes are all 2^60 - c, and the Shoup form for
everything else -- and most kernels are templated on LOGN1 (N = 1024 << LOGN1), so a (kernel, LOGN1, form) instantiation is machine code
of its own.  The prime-size rule (sec128 off) gives the chains below the Shoup form at every ring size:

    mixed     {60, 50, 40, 60}   engines [u64, u64, fp64, u64]: a 60-bit and a 50-bit prime in the Shoup u64 engine, an fp64 prime between
                                 them and the special prime, L = 3; every dual launch has both engines
    u64       {60, 50, 60}       no fp64 prime, hence no dual launches: the Shoup u64 engine's own grids
    forced    {60, 45, 45, 60}   under HE355_FORCE_U64=1: 45-bit primes on the Shoup u64 engine (set around the context's creation only)

An entry gives N, the bit sizes, whether the u64 engine is forced, and the form and engines the chain must have.  `check` holds moduli a
context made to its entry through tests/explicit_moduli.py (form_of, is_f64); the GPU side also holds `g.fp64` to `engines`.  BFV
contexts take PLAIN_BITS (t = 1032193 at N = 8192, 786433 at N = 16384 and 32768)."""
from __future__ import annotations

import os

import explicit_moduli as xm

PLAIN_BITS = 20
MIXED = (60, 50, 40, 60)
U64 = (60, 50, 60)
FORCED = (60, 45, 45, 60)
PLAIN_T = {8192: 1032193, 16384: 786433, 32768: 786433}


def _e(N, bits, forced=False):
    fp64 = tuple(False for _ in bits) if forced else tuple(b <= 47 for b in bits)
    return {"N": N, "bits": tuple(bits), "forced": forced, "form": "shoup", "fp64": fp64}


RINGS = {
    "n8192_60_50_40_60_shoup": _e(8192, MIXED),
    "n16384_60_50_40_60_shoup": _e(16384, MIXED),
    "n32768_60_50_40_60_shoup": _e(32768, MIXED),
    "n16384_60_50_60_shoup": _e(16384, U64),
    "n16384_60_45_45_60_forced_shoup": _e(16384, FORCED, True),
}


def bits(name):
    return list(RINGS[name]["bits"])


def spec(name):
    """(N, bit sizes, plain bits): the triple the BFV tables hold"""
    return RINGS[name]["N"], bits(name), PLAIN_BITS


def engines(name, moduli):
    """the fp64 flags the device must report for this entry: explicit_moduli.is_f64 per prime, none under a forced u64 engine"""
    return [False] * len(moduli) if RINGS[name]["forced"] else [xm.is_f64(q) for q in moduli]


def form(name, moduli):
    """the form of the u64 engine as the library picks it: over the primes that engine holds (every prime when it is forced)"""
    if not RINGS[name]["forced"]:
        return xm.form_of(moduli)
    return "fold" if all(xm.fold_prime_ok(q) for q in moduli) else "shoup"


def check(name, moduli, t=None):
    """the chain a context made is the entry's: its bit sizes, the Shoup form, the table's engines (and the plain modulus of PLAIN_BITS)"""
    e = RINGS[name]
    assert xm.bits_of(moduli) == list(e["bits"]), (name, xm.bits_of(moduli))
    assert form(name, moduli) == e["form"] == "shoup", (name, "the form of the u64 engine", form(name, moduli))
    assert tuple(engines(name, moduli)) == e["fp64"], (name, engines(name, moduli))
    assert not all(e["fp64"]), (name, "no prime in the u64 engine")
    if t is not None:
        assert t == PLAIN_T[e["N"]], (name, t)


def check_device(name, g):
    """the device context of an entry: the chain, and he355_prime_uses_fp64 against the restated engine rule"""
    check(name, g.moduli)
    assert list(g.fp64) == engines(name, g.moduli), (name, g.fp64)


class forced_u64:
    """HE355_FORCE_U64=1 around the creation of a context, restored afterwards (a no-op for an entry that does not force the engine)"""

    def __init__(self, name):
        self.on = RINGS[name]["forced"]

    def __enter__(self):
        self.old = os.environ.get("HE355_FORCE_U64")
        if self.on:
            os.environ["HE355_FORCE_U64"] = "1"
        return self

    def __exit__(self, *exc):
        if self.on:
            if self.old is None:
                os.environ.pop("HE355_FORCE_U64", None)
            else:
                os.environ["HE355_FORCE_U64"] = self.old
        return False
