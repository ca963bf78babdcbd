"""The (LOGN1, form) instantiations the GPU suite runs, family by family (no GPU: the tables are read, nothing is launched).

Every file with device code is built twice -- the fold form, for chains whose u64-engine primes are all 2^60 - c, and the Shoup form for
everything else -- and most kernels are templated on LOGN1 (N = 1024 << LOGN1): a (kernel, LOGN1, form) instantiation is machine code of
its own.  This module reads the context tables of the table-driven GPU modules and their helpers, builds every chain's moduli in the
oracle (the prime-size rule, sec128 off; a chain given by its primes is taken as it is), derives (LOGN1, form, has fp64, has u64) with
the rules of tests/explicit_moduli.py and asserts that each family holds a context in every cell of LOGN1 in {3, 4, 5} x {fold, shoup}.
A cell left empty on purpose is an entry of EXCEPTIONS with its reason, and an exception whose cell has been filled since is an error
too, so the list cannot outlive its reasons.  The matrix is printed (shown with -s).

The tables are read as the modules define them; importing a GPU test module touches no device (their contexts are made in fixtures)."""
import importlib

import bfv_gpu_helpers as bh
import bfv_multiply_plan as mp
import client_operands as co
import explicit_moduli as xm
import hoisted_layouts as hl
import launch_plan as lp

LOGN1S = (3, 4, 5)
FORMS = ("fold", "shoup")


def _mod(name):
    return importlib.import_module(name)


def evaluator():
    """(context, scheme, N, bits or primes, forced): test_gpu_parity.CONFIGS and launch_plan.CHAINS"""
    rows = [(f"test_gpu_parity:{k}", "ckks", N, bits, force) for k, (N, bits, force) in _mod("test_gpu_parity").CONFIGS.items()]
    return rows + [(f"launch_plan:{k}", scheme, N, list(bits), False) for k, (scheme, N, bits) in lp.CHAINS.items()]


def edge_operands():
    return [(f"test_gpu_edge_operands:{k}", "ckks", N, bits, force) for k, (N, bits, force) in _mod("test_gpu_edge_operands").CHAINS.items()]


def behz_multiply():
    return [(f"bfv_multiply_plan:{k}", "bfv", N, list(bits), force) for k, ((N, bits, _), force, *_) in mp.CHAINS.items()]


def pir_large_rings():
    rows = []
    for k, c in _mod("test_gpu_bfv_large_rings").CHAINS.items():
        N, bits, _ = bh.ALL[c] if isinstance(c, str) else c
        rows.append((f"test_gpu_bfv_large_rings:{k}", "bfv", N, list(bits), False))
    return rows


def pir_layouts():
    """test_gpu_bfv_chain_layouts.LAYOUTS, and bfv_gpu_helpers.ALL: the chains of the level, NTT-form and noise modules (mod_switch, the
    plain operands, to / from NTT form, the plain inner product, the noise budget)"""
    rows = [(f"test_gpu_bfv_chain_layouts:{k}", "bfv", N, list(bits), False) for k, ((N, bits, _), *_) in _mod("test_gpu_bfv_chain_layouts").LAYOUTS.items()]
    return rows + [(f"bfv_gpu_helpers.ALL:{k}", "bfv", N, list(bits), False) for k, (N, bits, _) in bh.ALL.items()]


def hoisted():
    rows = []
    for k in hl.LAYOUTS:
        e = hl.entry(k)
        rows.append((f"hoisted_layouts:{k}", e["scheme"], e["N"], e["primes"] if e["primes"] is not None else e["bits"], False))
    rh = _mod("test_gpu_rotate_hoisted")
    rows += [(f"test_gpu_rotate_hoisted:{k}", "ckks", N, bits, force) for k, (N, bits, force) in rh.CKKS.items()]
    return rows + [(f"test_gpu_rotate_hoisted:bfv_{k}", "bfv", N, bits, False) for k, (N, bits, _) in rh.BFV.items()]


def client():
    rows = [(f"test_gpu_client:{k}", scheme, N, bits, False) for k, (scheme, N, bits, _) in _mod("test_gpu_client").CASES.items()]
    return rows + [(f"client_operands.ENCRYPT_CHAINS:{k}", scheme, N, bits, False) for k, (scheme, N, bits, _) in co.ENCRYPT_CHAINS.items()]


FAMILIES = {"evaluator": evaluator, "edge operands": edge_operands, "BEHZ multiply": behz_multiply, "PIR large rings": pir_large_rings,
            "PIR layouts": pir_layouts, "hoisted": hoisted, "client": client}

# (family, LOGN1, form): why no context of the family's tables lies in the cell
EXCEPTIONS = {
    # tests/test_gpu_edge_operands.py argues about magnitudes -- accumulation runs, digit rows, floor edges -- that do not depend on the
    # ring; its table stops at N = 4096 apart from the all-fp64 chain at N = 32768 (no u64 engine, hence no form) and the Shoup chain at
    # N = 16384.  The fold form at N = 32768 runs in its test_headline_chain, which builds its context outside the table.
    ("edge operands", 3, "fold"): "the table's fold chains stop at N = 4096: the operand families are ring-independent",
    ("edge operands", 4, "fold"): "as at LOGN1 = 3",
    ("edge operands", 5, "fold"): "test_headline_chain runs {60, 45 x 15, 60} at N = 32768 outside the table",
    ("edge operands", 3, "shoup"): "one Shoup ring was asked of this module, N = 16384; each further ring costs nine tests with closed forms in Python integers",
    ("edge operands", 5, "shoup"): "as at LOGN1 = 3",
    # tests/test_gpu_bfv_chain_layouts.py is about engine layouts at the smallest ring with a column pass, and test_gpu_bfv_large_rings.py
    # owns the fused calls at LOGN1 >= 3 in both forms.  The fold cells at LOGN1 = 3 and 5 are held by bfv_gpu_helpers.ALL alone (the
    # level, NTT-form and noise calls); select, the selectors, merge and the reply pair run at N >= 8192 on the one Shoup ring, N = 16384,
    # and nowhere in the fold form: open, see DESIGN.md.
    ("PIR layouts", 4, "fold"): "no chain of ALL or of the layouts is N = 16384 in the fold form; the fused calls there are test_gpu_bfv_large_rings.py's",
    ("PIR layouts", 3, "shoup"): "one Shoup ring, N = 16384, runs every call of these modules; the other rings are open",
    ("PIR layouts", 5, "shoup"): "as at LOGN1 = 3",
}

_MODULI = {}


def moduli_of(oracle, scheme, N, bits):
    """the chain a context of (scheme, N, bits) holds, from the oracle (once per chain); primes themselves pass through"""
    if max(bits) > 60:
        return [int(q) for q in bits]
    key = (scheme, N, tuple(bits))
    if key not in _MODULI:
        if scheme == "ckks":
            o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=list(bits), sec128=False)
        else:
            o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=list(bits), plain_bits=20, sec128=False)
        _MODULI[key] = [int(q) for q in o.moduli]
        assert xm.bits_of(_MODULI[key]) == list(bits), key
    return _MODULI[key]


def cell_of(moduli, N, forced):
    """(LOGN1, form, has fp64, has u64): HE355_FORCE_U64=1 puts every prime on the u64 engine, whose form is then taken over all of them"""
    f64 = [False] * len(moduli) if forced else [xm.is_f64(q) for q in moduli]
    wide = [q for q, f in zip(moduli, f64) if not f]
    form = None if not wide else "fold" if all(xm.fold_prime_ok(q) for q in wide) else "shoup"
    return N.bit_length() - 11, form, any(f64), bool(wide)


def matrix(oracle, tables=FAMILIES):
    """{family: {(LOGN1, form): [(context, has fp64, has u64)]}}"""
    out = {}
    for fam, rows in tables.items():
        cells = out.setdefault(fam, {})
        for name, scheme, N, bits, forced in rows():
            logn1, form, has_f, has_u = cell_of(moduli_of(oracle, scheme, N, bits), N, forced)
            cells.setdefault((logn1, form), []).append((name, has_f, has_u))
    return out


def render(m):
    lines = [f"{'family':16s} " + " ".join(f"{f'LOGN1={l} {f}':>15s}" for l in LOGN1S for f in FORMS) + "   (contexts; b: one of them has both engines)"]
    for fam, cells in m.items():
        row = []
        for l in LOGN1S:
            for f in FORMS:
                got = cells.get((l, f), [])
                row.append(f"{str(len(got)) + ('b' if any(hf and hu for _, hf, hu in got) else ''):>15s}" if got else f"{'-':>15s}")
        lines.append(f"{fam:16s} " + " ".join(row))
    return "\n".join(lines)


def test_every_family_runs_every_ring_size_in_both_forms(oracle):
    m = matrix(oracle)
    print()
    print(render(m))
    for fam, cells in m.items():
        for l in LOGN1S:
            for f in FORMS:
                for name, _, _ in cells.get((l, f), []):
                    print(f"  {fam:16s} LOGN1={l} {f:5s} {name}")
    empty = [(fam, l, f) for fam in FAMILIES for l in LOGN1S for f in FORMS if not m[fam].get((l, f))]
    unexplained = [c for c in empty if c not in EXCEPTIONS]
    assert not unexplained, ("no context of the family's tables runs these (family, LOGN1, form) instantiations", unexplained)
    stale = [c for c in EXCEPTIONS if c not in empty]
    assert not stale, ("these cells hold a context now: take their exceptions out", stale)
    for c in empty:
        print(f"  empty {c}: {EXCEPTIONS[c]}")


def test_the_shoup_cells_hold_both_engines_where_the_family_has_dual_launches(oracle):
    """a Shoup cell filled by u64-only chains would leave the dual launches' Shoup halves unrun: in every filled Shoup cell at LOGN1 >= 3 one
    context has an fp64 prime beside the u64 ones"""
    m = matrix(oracle)
    for fam, cells in m.items():
        for l in LOGN1S:
            got = cells.get((l, "shoup"), [])
            assert not got or any(hf and hu for _, hf, hu in got), (fam, l, got)


def test_the_rules_of_the_cells():
    q60, q50, q40 = 0xffffffffffd8001, 0x3ffffffdf0001, 0xffffe80001  # N = 16384: the largest primes 1 (mod 2N) below 2^60, 2^50, 2^40
    assert cell_of([q60, q50, q40, q60], 16384, False) == (4, "shoup", True, True)
    assert cell_of([q60, q40, q60], 16384, False) == (4, "fold", True, True)
    assert cell_of([q60, q40, q60], 16384, True) == (4, "shoup", False, True)  # forced: the 40-bit prime joins the u64 engine
    assert cell_of([q40, q40], 8192, False) == (3, None, True, False) and cell_of([q60], 32768, False) == (5, "fold", False, True)
    assert cell_of([q60, q50], 1024, False)[0] == 0 and cell_of([q60, q50], 4096, False)[0] == 2
