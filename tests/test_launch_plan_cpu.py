"""tests/launch_plan.py -- the library's kernel-selection rules restated in Python -- pinned to what the product's comments, profiles/
and tests/test_gpu_bench_shapes.py state, and the completeness of the case table of tests/test_gpu_selection_boundaries.py: over that
table every selection decision takes every one of its outcomes at least once.  The restatement itself is held to the product's text:
the shape rule to csrc/ks_shape.h and every launcher's grids to csrc/ks_launch.h through the entry points of tests/csim/sim_rules.cpp,
cell by cell over every chain, level and batch the restatement was built for, and the four host headers of the device context's rules
at their edges under the sanitizers (tests/shape_rules_main.cpp).
No GPU, and the device library is not loaded."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csim_lib  # noqa: E402
import launch_plan as lp  # noqa: E402
import sanitized_program  # noqa: E402

HEADLINE = lp.chain("ckks", 32768, lp.HEADLINE_BITS)


def shapes(ch, L, ns, kind="product", apart=True):
    return [lp.ks_shape(ch, L, n, kind, apart) for n in ns]


def test_engine_rule_matches_the_chains_the_gpu_tests_assert():
    # tests/test_gpu_bench_shapes.py::ONE_ENGINE_SHAPES asserts Context.fp64 of these chains on the device
    assert lp.engines([60, 60, 60]) == (False, False, False)
    assert lp.engines([60, 45, 45, 60]) == (False, True, True, False)
    assert lp.engines([47, 46, 45, 44, 47]) == (True,) * 5


def test_headline_boundaries():
    # ks_shape.h, lat_limit / fuse_pays: N = 2^15 crosses between 4 and 5 ciphertexts; fused from 17 at L = 16 instead of 25
    assert lp.lat_limit(HEADLINE) == 4
    assert shapes(HEADLINE, 16, [4, 5, 16, 17]) == ["latency", "unfused", "unfused", "fused"]
    for L in (15, 12, 11, 6, 1):
        assert shapes(HEADLINE, L, [4, 5, 17, 24, 25]) == ["latency", "unfused", "unfused", "unfused", "fused"], L
    # at n = 17 the boundary lies between L = 15 and L = 16
    assert not lp.fuse_pays(HEADLINE, 17, 15) and lp.fuse_pays(HEADLINE, 17, 16)
    # N = 2^14, L = 4: 8 / 9 and 56 / 57
    ch = lp.chain("ckks", 16384, [60, 45, 45, 45, 60])
    assert shapes(ch, 4, [8, 9, 56, 57]) == ["latency", "unfused", "unfused", "fused"]


def test_lds_limits():
    # ks_shape.h, lds_limit: 64 ciphertexts at {60, 40, 60}, 32 at {60, 40, 40, 60} (N = 8192); profiles/r06_lds_shape.txt
    assert lp.lds_limit(lp.chain("ckks", 8192, [60, 40, 60]), 2) == 64
    assert lp.lds_limit(lp.chain("ckks", 8192, [60, 40, 40, 60]), 3) == 32
    ch = lp.chain("ckks", 2048, [46, 40, 40, 46])  # the n2048_f64 chain
    assert lp.lds_limit(ch, 3) == 128 and shapes(ch, 3, [128, 129]) == ["lds", "unfused"]
    # N = 8192, {60, 45, 60}: LDS to 64, unfused to 120, fused from 121; with `out` over an operand the latency shape to 12
    ch = lp.chain("ckks", 8192, [60, 45, 60])
    assert shapes(ch, 2, [64, 65, 120, 121]) == ["lds", "unfused", "unfused", "fused"]
    assert shapes(ch, 2, [12, 13, 120, 121], apart=False) == ["latency", "unfused", "unfused", "fused"]
    assert not lp.lds_supported(HEADLINE, 16) and not lp.lds_supported(lp.chain("ckks", 8192, [60] + [45] * 7 + [60]), 7)
    # grouped key switches choose between the fused and unfused shapes only
    assert shapes(ch, 2, [1, 5, 64], kind="grouped") == ["unfused"] * 3


def test_level_sum_pays_at_the_bench_shapes():
    # tests/test_gpu_bench_shapes.py: configs[4] (64 ciphertexts, BFV {60,40,40,60}, N = 2^15) forms its level sums in k_k3 at the default
    # chunk and at chunk 5 x 64, by k_sum_groups at chunk 32; 128 ciphertexts at N = 2^14, L = 2 form them in k_k3
    ch = lp.chain("bfv", 32768, [60, 40, 40, 60])
    assert lp.level_sum_pays(ch, 3, 64) and lp.level_sum_pays(ch, 3, 64, chunk=320) and not lp.level_sum_pays(ch, 3, 64, chunk=32)
    p = lp.plan_call(ch, "rotate_sum", 3, 64, steps=[j * 128 for j in range(1, 128)], key_steps=[1 << k for k in range(15)] + [-(1 << k) for k in range(15)])
    assert p.key_switches == 127 and p.level_sums_by_kernel == 0 and p.level_sums_in_k3 >= 4
    for bits in ([60, 60, 60], [45, 45, 60]):
        ch = lp.chain("ckks", 16384, bits)
        assert lp.level_sum_pays(ch, 2, 128)
        p = lp.plan_call(ch, "rotate_sum", 2, 128, steps=[1, 2, 3], key_steps=[1, -1, 2, -2, 4, -4])
        assert p.level_sums_in_k3 == 2 and p.level_sums_by_kernel == 0
        # (every data prime on one engine: the data-prime launch is that engine's k_k3 alone)
        assert all(l.family == "k_k3" for l in p.launches() if l.family.startswith("k_k3"))
    assert not lp.level_sum_pays(lp.chain("ckks", 16384, [60, 60, 60]), 2, 127)


def test_dot_bench_shape_runs_k_k3_dual8():
    # tests/test_gpu_bench_shapes.py: configs[3] at n = 64 runs k_k3_dual8, every key switch fused (1 relinearization + 12 rotations)
    for op in ("multiply_relin", "apply_galois"):
        p = lp.plan_call(HEADLINE, op, 16, 64)
        assert p.counters()["ks_fused"] == 1 and sum(p.counters().values()) == 1
        data = [l for l in p.launches() if l.family.startswith("k_k3") and "data primes" in l.note]
        assert [l.family for l in data] == ["k_k3_dual8"] and data[0].grid[0] <= lp.DUAL_MAX_BLOCKS_K3
    # one ciphertext more per op-group row and the engines part
    assert ("k_k3", "separate") in lp.outcomes(HEADLINE, lp.plan_call(HEADLINE, "multiply_relin", 16, 65))


def test_wide_digit_grid_takes_one_launch_per_engine():
    # tests/test_gpu_bench_shapes.py::ONE_ENGINE_SHAPES["wide_digit_grid"]: 256 x 3 digits x 4 > 1024 blocks, k_k2n per digit kind; fused
    ch = lp.chain("ckks", 4096, [60, 45, 45, 60])
    p = lp.plan_call(ch, "multiply_relin_rescale", 3, 256)
    assert p.counters()["ks_fused"] == 1
    fam = [l.family for l in p.launches()]
    assert fam.count("k_k2n") == 2 and "k_k2n_dual" not in fam and fam.count("k_k1") == 2 and "k_k1_dual" not in fam
    # latency shape on the u64 engine alone: k_k1 / k_k2n / k_k3 of that engine
    ch = lp.chain("ckks", 16384, [60, 60, 60])
    p = lp.plan_call(ch, "multiply_relin_rescale", 2, 2)
    assert p.counters()["ks_latency"] == 1 and not any(l.family.endswith(("dual", "dual8")) for l in p.launches())


def test_grids_stay_inside_the_launch():
    """every planned launch has blocks, and a k_k3 grid holds a whole number of 8-tile groups per op-group block"""
    for name, op, L, ns in lp.case_table():
        ch = lp.case_chain(name)
        for n in ns:
            for l in lp.plan_call(ch, op, L, n).launches():
                assert l.grid[0] > 0 and l.grid[1] > 0 and l.block in (64, 256, 512, 64 << ch.logn1), (name, op, n, l)
                if l.family == "k_k3" and l.waves > 1:
                    assert l.grid[0] % 8 == 0, (name, op, n, l)


def test_case_table_takes_every_outcome_of_every_decision():
    """The completeness condition: over the case table (the mixed-shape calls included) every decision takes each of its outcomes at
    least once.  A decision may be unreachable only if no chain with N <= 32768 and n <= 512 reaches it; none is."""
    seen, lines = {}, []
    for name, op, L, ns in lp.case_table():
        ch = lp.case_chain(name)
        lines.append(f"{name:32s} {op:30s} L={L:<2d} n = {ns}")
        for n in ns:
            p = lp.plan_call(ch, op, L, n)
            oc = lp.outcomes(ch, p)
            for o in oc:
                seen.setdefault(o, (name, op, L, n))
            lines.append(f"    n={n:<4d} {lp.describe(ch, p)[:230]}")
    name = "n8192_60_45_60_both_engines"
    ch = lp.case_chain(name)
    for op, chunk, n in lp.mixed_shape_calls(ch, ch.Ltop):
        p = lp.plan_call(ch, op, ch.Ltop, n, chunk)
        got = {c.shape for c in p.chunks}
        assert len(got) == 2 and got & {"lds", "latency"} and got & {"unfused", "fused"}, (op, chunk, n, got)
        lines.append(f"{name:32s} {op:30s} chunk={chunk} n={n}: {[c.shape for c in p.chunks]}")
    print()  # (shown with -s)
    print("\n".join(lines))
    print("\nfirst case that takes each outcome:")
    for d, outs in lp.DECISIONS.items():
        for o in outs:
            print(f"  {d:13s} {str(o):15s} {seen.get((d, o), 'UNREACHED')}")
    missing = [(d, o) for d, outs in lp.DECISIONS.items() for o in outs if (d, o) not in seen]
    assert not missing, missing
    assert (72, 149) in [(c, n) for _, c, n in lp.mixed_shape_calls(ch, ch.Ltop)]  # chunk 72 with n = 2 x 72 + 5 at {60,45,60}, N = 8192


def test_shoup_rows_of_the_case_table():
    """The rows that run the Shoup build of the u64 engine at N >= 8192: their chains are entries of tests/shoup_rings.py under the same
    names (bit sizes, ring, engines), the selection rules do not look at the form -- the same boundaries as a fold chain of the same
    length -- and between them the rows reach every shape the ring admits, with both engines in every dual rule at {60, 50, 40, 60}."""
    import shoup_rings as sr
    assert lp.SHOUP_CHAINS == ("n16384_60_50_40_60_shoup", "n8192_60_50_40_60_shoup", "n16384_60_50_60_shoup")
    for name in lp.SHOUP_CHAINS:
        scheme, N, bits = lp.CHAINS[name]
        e = sr.RINGS[name]
        assert scheme == "ckks" and (N, bits) == (e["N"], e["bits"]) and lp.engines(bits) == e["fp64"] and not e["forced"], name
    rows = {}
    for name, op, L, ns in lp.case_table():
        if name in lp.SHOUP_CHAINS:
            rows.setdefault(name, {})[op] = (L, ns)
    assert sorted(rows["n16384_60_50_40_60_shoup"]) == ["apply_galois", "multiply_relin_rescale", "multiply_relin_rescale_over_a", "relinearize",
                                                        "rotate_each", "rotate_sum"]
    assert sorted(rows["n8192_60_50_40_60_shoup"]) == ["multiply_relin_rescale", "relinearize_rescale", "rotate_add_in_place", "rotate_sum"]
    assert sorted(rows["n16384_60_50_60_shoup"]) == ["multiply_relin_rescale", "rotate_sum"]
    # N = 2^14, L = 3: latency to 8, unfused to 56, fused from 57 (16 x ceil(n / 8) >= 128); L = 2 on the u64 engine alone: the same
    ch = lp.case_chain("n16384_60_50_40_60_shoup")
    assert ch.logn1 == 4 and shapes(ch, 3, [8, 9, 56, 57]) == ["latency", "unfused", "unfused", "fused"]
    assert shapes(ch, 3, [8, 9, 56, 57], apart=False) == ["latency", "unfused", "unfused", "fused"]
    assert rows["n16384_60_50_40_60_shoup"]["multiply_relin_rescale"] == (3, [1, 8, 9, 10, 11, 15, 16, 17, 21, 22, 40, 41, 56, 57, 63, 64, 65, 85, 86])
    assert rows["n16384_60_50_40_60_shoup"]["rotate_sum"] == (3, [1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 18, 19, 23, 24, 25, 28, 29, 87, 88, 256, 257])
    u = lp.case_chain("n16384_60_50_60_shoup")
    assert shapes(u, 2, [8, 9, 56, 57]) == ["latency", "unfused", "unfused", "fused"]
    assert rows["n16384_60_50_60_shoup"]["multiply_relin_rescale"] == (2, [1, 8, 9, 15, 16, 17, 32, 33, 40, 41, 56, 57, 63, 64, 65, 128, 129])
    # N = 8192, L = 3: the ring-in-LDS shape to 32 (384 / 12), unfused to 120, fused from 121
    c8 = lp.case_chain("n8192_60_50_40_60_shoup")
    assert c8.logn1 == 3 and lp.lds_limit(c8, 3) == 32 and shapes(c8, 3, [32, 33, 120, 121]) == ["lds", "unfused", "unfused", "fused"]
    assert rows["n8192_60_50_40_60_shoup"]["multiply_relin_rescale"] == (3, [1, 32, 33, 36, 37, 39, 40, 41, 80, 81, 85, 86, 120, 121, 127, 128, 129])
    for name, want in (("n16384_60_50_40_60_shoup", {"latency", "unfused", "fused"}), ("n8192_60_50_40_60_shoup", {"lds", "unfused", "fused"}),
                       ("n16384_60_50_60_shoup", {"latency", "unfused", "fused"})):
        ch = lp.case_chain(name)
        dual = set()
        for op, (L, ns) in rows[name].items():
            got = {c.shape for n in ns for c in lp.plan_call(ch, op, L, n).chunks}
            assert got == want, (name, op, got)  # every shape the chain reaches is run -- and asserted through he355_path_stats -- per op
            dual |= {l.family for n in ns for l in lp.plan_call(ch, op, L, n).launches() if l.family.endswith(("dual", "dual8"))}
        if name == "n16384_60_50_60_shoup":
            assert dual == {"k_k2n_dual"}, dual  # no fp64 prime: no launch for both engines; k_k2n_dual pairs the two digit kinds (60 / 50 bits)
        else:
            assert dual >= {"k_k1_dual", "k_k3_dual8", "k_floor_rows_dual"}, (name, dual)
    assert max(ns[-1] for r in rows.values() for _, ns in r.values()) <= 257  # (the largest batch: 257 ciphertexts of 3 x 16384 words a polynomial)


def test_rotation_terms_and_trie():
    assert lp.naf_terms(3, 8192) == [-1, 4] and lp.naf_terms(5, 8192) == [1, 4] and lp.naf_terms(-3, 8192) == [1, -4]
    assert lp.rotation_terms(3, 8192, (1, 2, 4, -1)) == [-1, 4] and lp.rotation_terms(2, 8192, (1, 2, 4, -1)) == [2]
    assert lp.rotation_trie_levels((1, 2, 3), 8192, (1, 2, 4, -1)) == [3, 1]
    assert lp.galois_elt(1, 8192) == 3 and lp.galois_elt(0, 8192) == 16383 and lp.galois_elt(-1, 8192) == pow(3, 4095, 16384)


# ---- the restatement held to csrc/ks_shape.h ---------------------------------------------------------------------------------------------
SHAPES = ("lds", "latency", "fused", "unfused", "bfv_coeff")  # KsShape, in order
KINDS = ("product", "size3", "galois", "grouped")             # KsKind, in order
SCHEME_BFV, SCHEME_CKKS = 1, 2
AUTO, NEVER = 2 ** 64 - 1, 0  # what he355_set_latency_max / he355_set_lds_max take: 2^64 - 1 is "back to the rule", 0 "never"
HUGE = 2 ** 64 - 2            # the largest limit that IS a limit (no call of the suite sets it: it shows the rule's other conditions alone)


def limits(lat=AUTO, lds=AUTO, chunk=lp.DEFAULT_CHUNK):
    """{latency max, LDS max, chunk}: the two limits as the API takes them, mapped by KsLimits' own setters (sim_rules.cpp: limits_of)"""
    return (C.c_uint64 * 3)(lat, lds, chunk)


@pytest.fixture(scope="module")
def rules():
    S = csim_lib.load()
    u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    S.sim_ks_shape.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, u64p, C.c_int, C.c_uint64, C.c_int, C.c_int]
    S.sim_lat_limit.restype = C.c_uint64
    S.sim_lat_limit.argtypes = [C.c_uint64, C.c_int, u64p]
    S.sim_lds_limit.restype = C.c_uint64
    S.sim_lds_limit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, u64p, C.c_int]
    S.sim_ks_scan.restype = C.c_uint64
    S.sim_ks_scan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, u64p, C.c_int, C.c_uint64, u64p, C.c_size_t, u8p, u8p, u8p, u64p, u8p]
    i32p = C.POINTER(C.c_int32)
    S.sim_kl_consts.restype = None
    S.sim_kl_consts.argtypes = [i32p]
    S.sim_kl_scan.restype = None
    S.sim_kl_scan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u8p, u64p, C.c_int, C.c_uint64, i32p, C.c_size_t, i32p]
    return S


def test_shape_rule_equals_the_header_over_every_chain_level_and_batch(rules):
    """lp.ks_shape, fuse_pays, level_sum_pays, lat_limit, lds_limit and lds_supported against csrc/ks_shape.h: every chain of lp.CHAINS,
    L = 1 .. L_top, n = 1 .. lp.SCAN_MAX, the four kinds, `out` apart or not; level_sum_pays at the default chunk, at the chunks of this
    module's own cases and at those of the mixed-shape calls.  The environment is the NTT-domain pipeline's (scheme CKKS: what
    batch_env(0, true) makes of a BFV context too), which is where every planned launch runs; one filled array per chain."""
    mixed = lp.case_chain("n8192_60_45_60_both_engines")
    chunks = sorted({lp.DEFAULT_CHUNK, 320, 32} | {c for _, c, _ in lp.mixed_shape_calls(mixed, mixed.Ltop)})
    nmax = lp.SCAN_MAX
    for name in lp.CHAINS:
        ch = lp.case_chain(name)
        Lt = ch.Ltop
        shape, fuse = (C.c_uint8 * (Lt * nmax * 8))(), (C.c_uint8 * (Lt * nmax))()
        lsum = (C.c_uint8 * (len(chunks) * Lt * nmax))()
        lds_lim, lds_ok = (C.c_uint64 * Lt)(), (C.c_uint8 * Lt)()
        lat = rules.sim_ks_scan(SCHEME_CKKS, ch.logn1, ch.K, ch.N, ch.K, limits(), Lt, nmax, (C.c_uint64 * len(chunks))(*chunks), len(chunks),
                                shape, fuse, lsum, lds_lim, lds_ok)
        assert lat == lp.lat_limit(ch), name
        for L in range(1, Lt + 1):
            assert lds_lim[L - 1] == lp.lds_limit(ch, L) and bool(lds_ok[L - 1]) == lp.lds_supported(ch, L), (name, L)
            for n in range(1, nmax + 1):
                at = (L - 1) * nmax + n - 1
                assert bool(fuse[at]) == lp.fuse_pays(ch, n, L), (name, L, n)
                for k, kind in enumerate(KINDS):
                    for apart in (False, True):
                        assert SHAPES[shape[(at * 4 + k) * 2 + apart]] == lp.ks_shape(ch, L, n, kind, apart), (name, L, n, kind, apart)
                for ci, c in enumerate(chunks):
                    assert bool(lsum[ci * Lt * nmax + at]) == lp.level_sum_pays(ch, L, n, c), (name, L, n, c)


# ---- the launch geometry held to csrc/ks_launch.h ------------------------------------------------------------------------------------------
K3_ALL, K3_SPECIAL, K3_DATA = 0, 1, 2  # K3Part, in order
AT_L, AT_L1, NO_TAIL = -1, -2, -100      # level arguments of sim_kl_scan: L, L - 1; no tail prime
GS_N = -1                              # group size: the batch itself (rotate_sum: one group per trie node)
PARTS = {K3_ALL: "all", K3_SPECIAL: "special", K3_DATA: "data"}
# launch_k3 as plan_chunk issues it: {part, fuse (3: with the rescale's second floor step), tt_lo, tt_hi, n_split, n_split_u64, group size, sum_out}
K3_COMBOS = (
    [(part, 0, 0, 0, 1, 0, 0, 0) for part in PARTS]                                         # unfused: all / special / data
    + [(K3_DATA, 1, 0, AT_L, 1, 0, 0, 0), (K3_DATA, 3, 0, AT_L1, 1, 0, 0, 0), (K3_DATA, 1, AT_L1, AT_L, 1, 0, 0, 0)]  # fused over [0, L), [0, L-1), [L-1, L)
    + [(K3_ALL, 0, 0, 0, lp.LAT_SPLIT, lp.LAT_SPLIT_U64, 0, 0)]                              # the latency splits
    + [c for gs in (1, GS_N) for c in ((K3_ALL, 0, 0, 0, 1, 0, gs, 0), (K3_SPECIAL, 0, 0, 0, 1, 0, gs, 0), (K3_DATA, 1, 0, AT_L, 1, 0, gs, 0))]  # grouped
    + [(K3_SPECIAL, 0, 0, 0, 1, 0, gs, 1) for gs in (8, GS_N)]                               # the special prime's launch ahead of a level sum
    + [(K3_DATA, 1, 0, AT_L, 1, 0, gs, 1) for gs in (1, 8, 12, GS_N)]                        # the level sum: groups of a multiple of eight or not
)
LAUNCHERS = {
    # name: (launcher code of sim_kl_scan, kernel families by form, the combinations, lp's plan of one combination)
    "launch_k1": (0, ("k_k1", "k_k1_dual"), [(c2,) for c2 in (0, 1)], None),
    "launch_k2": (1, ("k_k2n", "k_k2n_dual"), [(1,), (lp.LAT_TARGETS,)], lambda ch, L, n, c: lp.plan_k2(ch, L, n, c[0])),
    "launch_k3": (2, ("k_k3", "k_k3_dual", "k_k3_dual8"), K3_COMBOS, None),
    "launch_k3_combine": (3, ("k_k3_combine",), [()], lambda ch, L, n, c: lp.plan_k3_combine(ch, L, n)),
    "launch_floor_cols": (4, ("k_floor_colsn",), [(size, tgt, ts) for size in (2, 3) for tgt in (1, AT_L1, AT_L) for ts in (1, lp.LAT_TARGETS)], None),
    "launch_floor_rows": (5, ("k_floor_rows", "k_floor_rows_dual"), [(tgt, n_src, tail) for tgt in (AT_L, AT_L1) for n_src in (2, 3) for tail in (NO_TAIL, tgt - 1)], None),
    "launch_rows_inv_select": (6, ("k_rows_inv_select",), [(2,), (3,)], lambda ch, L, n, c: lp.plan_rows_inv_select(ch, n * c[0])),
}


def _level(L, v):
    return v if v >= 0 else L + 1 + v


def _plans(name, ch, L, n, c):
    """lp's plans of combination c of launcher `name`: [launches] per restated argument set that the combination stands for, or None where
    the restatement refuses the arguments"""
    if name == "launch_k1":  # the header reads one flag of (mode, no_c01): the ct x ct multiply that leaves c0, c1 to k_k3
        return [lp.plan_k1(ch, L, mode, n, no_c01) for mode in ("product", "size3", "galois") for no_c01 in (False, True)
                if (mode == "product" and no_c01) == bool(c[0])]
    if name == "launch_k3":
        part, fuse, lo, hi, n_split, n_split_u64, gs, sum_out = c
        try:
            return [lp.plan_k3(ch, L, n, PARTS[part], bool(fuse), _level(L, lo), _level(L, hi), n_split, n_split_u64, n if gs == GS_N else gs, bool(sum_out))]
        except AssertionError:
            return None
    if name == "launch_floor_cols":
        return [lp.plan_floor_cols(ch, n * c[0], _level(L, c[1]), c[2])]
    if name == "launch_floor_rows":
        return [lp.plan_floor_rows(ch, n, _level(L, c[0]), c[1], -1 if c[2] == NO_TAIL else _level(L, c[2]))]
    return [LAUNCHERS[name][3](ch, L, n, c)]


def _row(families, l):
    """one planned launch as sim_kl_scan's row"""
    form = families.index(l.family)
    og_u64 = int(l.note.split("u64")[1]) if form == 2 else 0
    engine = {"fp64": 1, "u64": 2}.get(l.engine, 0)
    if l.family == "k_k2n":
        engine = 2 if l.note == "60-bit digits" else 1
    return [form, l.grid[0], l.grid[1], l.block, l.og_per_block, og_u64, l.waves, l.ts, engine]


def test_launch_constants_are_the_headers(rules):
    out = (C.c_int32 * 7)()
    rules.sim_kl_consts(out)
    assert list(out) == [lp.K_WAVES, lp.K_BLOCK, lp.DUAL_MAX_BLOCKS, lp.DUAL_MAX_BLOCKS_K3, lp.LAT_TARGETS, lp.LAT_SPLIT, lp.LAT_SPLIT_U64]


@pytest.mark.parametrize("name", list(LAUNCHERS))
def test_launch_geometry_equals_the_header_over_every_chain_level_and_batch(rules, name):
    """lp.plan_k1, plan_k2 (_target_split), plan_k3 (_size_grid), plan_k3_combine, plan_floor_cols, plan_floor_rows and plan_rows_inv_select
    against csrc/ks_launch.h: every chain of lp.CHAINS, L = 1 .. L_top, n = 1 .. lp.SCAN_MAX, every argument combination plan_chunk,
    plan_rescale_tail, _plan_rotate_sum and _plan_rotate_each can issue.  Per launch: the family (dual, dual8 or the engine's own), grid
    x and y, threads per block, op-groups per block (both sides of k_k3_dual8), waves, target split, engine.  The header reads moduli where
    the restatement reads bit sizes: a stand-in modulus of the stated bit length (only q >> 52 is read), engines from lp.engines."""
    code, families, combos, _ = LAUNCHERS[name]
    nmax, nc = lp.SCAN_MAX, len(combos)
    flat = (C.c_int32 * (nc * 8))(*[v for c in combos for v in tuple(c) + (0,) * (8 - len(c))])
    for cname in lp.CHAINS:
        ch = lp.case_chain(cname)
        Lt = ch.Ltop
        out = (C.c_int32 * (Lt * nmax * nc * 37))()
        rules.sim_kl_scan(code, SCHEME_CKKS, ch.logn1, ch.K, (C.c_uint8 * ch.K)(*ch.fp64), (C.c_uint64 * ch.K)(*[1 << (b - 1) for b in ch.bits]),
                          Lt, nmax, flat, nc, out)
        got = out[:]
        for L in range(1, Lt + 1):
            for n in range(1, nmax + 1):
                for ci, c in enumerate(combos):
                    at = (((L - 1) * nmax + n - 1) * nc + ci) * 37
                    plans = _plans(name, ch, L, n, c)
                    if plans is None:
                        assert got[at] == -1, (cname, L, n, c)
                        continue
                    for ls in plans:
                        want = [len(ls)] + [v for l in ls for v in _row(families, l)]
                        assert got[at:at + len(want)] == want, (cname, L, n, c, ls)


def test_shape_rule_with_the_limits_set(rules):
    """he355_set_latency_max / he355_set_lds_max (launch_plan.py has no overrides: literal expectations).  Limit 0: the shape is never taken.
    Limit 2^64 - 1: the rule applies again -- the same limits and the same shapes as a context nobody set a limit on.  A limit between:
    that batch and no larger; HUGE, the largest value that is a limit, leaves the rule's other conditions to decide alone.  And the two
    inputs are two: a BFV context's own environment has one shape whatever the limits."""
    ch = lp.case_chain("n8192_60_45_60_both_engines")  # N = 8192, L = 2: LDS to 64, latency to 12, unfused to 120, fused from 121
    def shape(n, lim, kind="product", apart=True, scheme=SCHEME_CKKS, L=2, c=ch):
        return SHAPES[rules.sim_ks_shape(scheme, c.logn1, c.K, c.N, c.K, lim, L, n, KINDS.index(kind), apart)]
    def lat_lds(lim, L=2):
        return rules.sim_lat_limit(ch.N, ch.K, lim), rules.sim_lds_limit(SCHEME_CKKS, ch.logn1, ch.K, ch.N, ch.K, lim, L)
    auto_rows = ["lds", "lds", "unfused", "unfused", "fused"]
    assert [shape(n, limits()) for n in (1, 64, 65, 120, 121)] == auto_rows and lat_lds(limits()) == (12, 64)
    # 2^64 - 1 handed to either setter, or to both: the AUTO rows again, not "every batch"
    for lim in (limits(lat=2 ** 64 - 1), limits(lds=2 ** 64 - 1), limits(lat=2 ** 64 - 1, lds=2 ** 64 - 1)):
        assert lat_lds(lim) == (12, 64)
        assert [shape(n, lim) for n in (1, 64, 65, 120, 121)] == auto_rows
        assert [shape(n, lim, apart=False) for n in (12, 13, 120, 121)] == ["latency", "unfused", "unfused", "fused"]
        assert shape(2 ** 40, lim) == "fused"
    assert lat_lds(limits(lat=NEVER, lds=2 ** 64 - 1)) == (0, 64) and lat_lds(limits(lat=2 ** 64 - 1, lds=NEVER)) == (12, 0)
    # limit 0: never
    assert [shape(n, limits(lds=NEVER)) for n in (1, 12, 13, 64, 121)] == ["latency", "latency", "unfused", "unfused", "fused"]
    assert [shape(n, limits(lds=NEVER, lat=NEVER)) for n in (1, 12, 120, 121)] == ["unfused", "unfused", "unfused", "fused"]
    assert [shape(n, limits(lat=NEVER)) for n in (1, 64, 65)] == ["lds", "lds", "unfused"]
    # a finite limit: that batch and no larger
    assert [shape(n, limits(lds=5, lat=7)) for n in (5, 6, 7, 8)] == ["lds", "latency", "latency", "unfused"]
    assert lat_lds(limits(lat=7, lds=5)) == (7, 5) and lat_lds(limits(lat=HUGE, lds=HUGE)) == (HUGE, HUGE)
    assert [shape(n, limits(lds=HUGE)) for n in (65, 121, 512, 2 ** 40)] == ["lds"] * 4
    assert [shape(n, limits(lds=HUGE), apart=False) for n in (12, 13, 121)] == ["latency", "unfused", "fused"]  # (`out` over an operand: never LDS)
    assert [shape(n, limits(lds=NEVER, lat=HUGE)) for n in (13, 121, 2 ** 40)] == ["latency"] * 3
    assert [shape(n, limits(lds=NEVER, lat=HUGE), kind="grouped") for n in (13, 121)] == ["unfused", "fused"]  # grouped: neither small shape
    # where the ring-in-LDS kernels do not exist no limit brings them: L = 7 of a nine-prime chain at N = 8192, any level at N = 2^14
    deep = lp.chain("ckks", 8192, [60] + [45] * 7 + [60])
    assert shape(1, limits(lds=HUGE), L=7, c=deep) == "latency" and shape(1, limits(lds=HUGE), L=6, c=deep) == "lds"
    wide = lp.case_chain("n16384_60_45_45_45_60_L4")
    assert shape(1, limits(lds=HUGE), L=4, c=wide) == "latency" and shape(9, limits(lds=HUGE), L=4, c=wide) == "unfused"
    # a BFV context's coefficient-form environment: one shape; the same context on the NTT-domain pipeline: the rule
    b = lp.case_chain("bfv_n8192_60_40_60")
    for lim in (limits(), limits(lds=HUGE, lat=HUGE), limits(lds=NEVER, lat=NEVER)):
        assert {shape(n, lim, kind=k, scheme=SCHEME_BFV, c=b) for n in (1, 64, 121) for k in KINDS} == {"bfv_coeff"}
    assert [shape(n, limits(), kind="galois", c=b) for n in (64, 65, 121)] == ["lds", "unfused", "fused"]


def test_the_rule_headers_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "shape_rules_main.cpp", "shape_rules ok")
