"""tests/launch_plan.py -- the library's kernel-selection rules restated in Python -- pinned to what the product's comments, profiles/
and tests/test_gpu_bench_shapes.py state, and the completeness of the case table of tests/test_gpu_selection_boundaries.py: over that
table every selection decision takes every one of its outcomes at least once.  Nothing of the product is compiled or loaded here."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_plan as lp  # noqa: E402

HEADLINE = lp.chain("ckks", 32768, lp.HEADLINE_BITS)


def shapes(ch, L, ns, kind="product", apart=True):
    return [lp.ks_shape(ch, L, n, kind, apart) for n in ns]


def test_engine_rule_matches_the_chains_the_gpu_tests_assert():
    # tests/test_gpu_bench_shapes.py::ONE_ENGINE_SHAPES asserts Context.fp64 of these chains on the device
    assert lp.engines([60, 60, 60]) == (False, False, False)
    assert lp.engines([60, 45, 45, 60]) == (False, True, True, False)
    assert lp.engines([47, 46, 45, 44, 47]) == (True,) * 5


def test_headline_boundaries():
    # he355_api.hip, lat_limit / fuse_pays: N = 2^15 crosses between 4 and 5 ciphertexts; fused from 17 at L = 16 instead of 25
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
    # he355_api.hip, lds_limit: 64 ciphertexts at {60, 40, 60}, 32 at {60, 40, 40, 60} (N = 8192); profiles/r06_lds_shape.txt
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
