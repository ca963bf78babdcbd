"""tests/bfv_multiply_plan.py -- the restatement of the BEHZ multiply's host-side kernel selection -- pinned to the numbers of the launchers
(csrc/he355_kernels_behz.hip) and to the operand-list geometry `bfv_multiply3` runs on (csrc/behz_lists.h, through tests/csim), and the case table of tests/test_gpu_bfv_multiply_routes.py shown to take
every outcome of every decision and each of the seven fused and two unfused instantiations at least once.  The auxiliary bases come from
the CPU build of the product's parameter code (tests/csim).  No GPU."""
import ctypes as C
import importlib
import os
import re

import pytest

import bfv_multiply_plan as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB = 1024


def level(N, bits, pb, L, **kw):
    return mp.levels(N, tuple(bits), pb, **kw)[L]


def test_auxiliary_base_sizes_and_the_lds_of_the_fused_kernels():
    """(L + nB + 1) x (64 << logn1) x 8 bytes: 72 and 88 KiB at N = 16384 need the runtime's opt-in, 64 KiB exactly does not"""
    for N, bits, pb, L, nB, kib in [(16384, [60, 40, 40, 40, 60], 20, 4, 4, 72), (16384, [60] * 5, 31, 3, 4, 64), (16384, [60] * 5, 31, 4, 6, 88),
                                    (16384, [60, 40, 40, 60], 20, 3, 3, 56), (16384, [60, 40, 40, 60], 20, 2, 2, 40), (16384, [60, 40, 40, 60], 20, 1, 2, 32),
                                    (4096, [60, 40, 40, 60], 20, 1, 1, 6), (8192, [60, 40, 40, 40, 60], 20, 1, 2, 16),
                                    (8192, [60] * 5, 20, 4, 5, 40), (8192, [60] * 5, 20, 2, 3, 24), (8192, [50, 40, 50], 20, 1, 1, 12)]:
        lv = level(N, bits, pb, L)
        assert (lv.nB, lv.lds_bytes) == (nB, kib * KIB), (N, bits, L, lv)
    # every fusable shape at N <= 8192 stays within 44 KiB: L <= 4, nB <= 6, 512 B per residue and row of 64 columns
    assert (4 + 6 + 1) * (64 << 3) * 8 == 44 * KIB and (4 + 6 + 1) * (64 << 4) * 8 == 88 * KIB


def test_the_fusable_rule_is_a_function_of_the_lds_limit():
    d4, x4 = level(16384, [60, 40, 40, 40, 60], 20, 4), mp.levels(16384, (60,) * 5, 31)
    for lv, kib in ((d4, 72), (x4[4], 88)):
        assert mp.fusable(lv, kib * KIB) and not mp.fusable(lv, kib * KIB - 1)
        assert mp.instantiation(lv, mp.LDS_MI355X) == "<4,4,6,false>" and mp.instantiation(lv, mp.LDS_NO_OPT_IN) == "<4,6>"
    assert mp.fusable(x4[3], mp.LDS_NO_OPT_IN) and x4[3].lds_bytes == mp.LDS_NO_OPT_IN  # exactly 64 KiB: no opt-in needed
    # a device that grants no more than 64 KiB: the plan of a call names the unfused route, and nothing else about the call changes
    fused, unfused = mp.plan(d4, 6, mp.GS_ALL, 2), mp.plan(d4, 6, mp.GS_ALL, 2, lds_limit=mp.LDS_NO_OPT_IN)
    assert (fused["cols_fused"], fused["cols_unfused"], unfused["cols_fused"], unfused["cols_unfused"], unfused["coef_wide"]) == (2, 0, 0, 2, 0)
    assert {k: v for k, v in fused.items() if not k.startswith("co")} == {k: v for k, v in unfused.items() if not k.startswith("co")}
    # L = 5 is never fused, whatever the ring; N = 1024 and N = 32768 have no fused kernel
    assert mp.instantiation(level(8192, [60, 40, 40, 40, 40, 60], 20, 5)) == "<16,24>"
    assert mp.instantiation(level(1024, [50, 40, 50], 20, 2)) == mp.instantiation(level(32768, [60, 40, 40, 60], 20, 3)) == "<4,6>"
    assert mp.instantiation(level(2048, [50, 40, 40, 45, 40, 60, 60], 22, 6)) == "<16,24>"


def test_the_1024_block_thresholds():
    """n_c (L + S) 2^logn1 <= 1024 per pair; ceil(3 n_c n_f 2^logn1 / 4) + ceil(3 n_c n_u 2^logn1 / 4) <= 1024 for the lists"""
    a = level(16384, [60, 40, 40, 60], 20, 3)
    assert (a.n_f, a.n_u, a.S) == (6, 1, 4) and mp.thresholds(a) == {"rows": (9, 10), "inv": (12, 13)}
    assert 9 * 7 * 16 == 1008 and 10 * 7 * 16 == 1120 and 12 * (72 + 12) == 1008 and 13 * (72 + 12) == 1092
    b = level(8192, [60, 40, 60], 20, 2)
    assert (b.n_f, b.n_u, b.S) == (4, 1, 3) and mp.thresholds(b) == {"rows": (25, 26), "inv": (34, 35)}
    assert 25 * 5 * 8 == 1000 and 26 * 5 * 8 == 1040 and 34 * (24 + 6) == 1020 and 35 * (24 + 6) == 1050
    # one engine for every residue: no dual launch at any size
    u = level(8192, [60, 40, 60], 20, 2, force_u64=True)
    assert (u.n_f, u.n_u) == (0, 5) and mp.thresholds(u) == {"rows": None, "inv": None}
    assert not mp.rows_dual(u, 1) and not mp.inv_dual(u, 1)
    s = level(8192, [60, 40, 60], 20, 2, seal_base=True)  # SEAL's 61-bit auxiliary primes: only the 40-bit data prime is left on the fp64 engine
    assert (s.n_f, s.n_u, s.nB) == (1, 4, 2)


def test_lists_or_per_pair():
    assert not mp.takes_lists(1, 1, 1) and not mp.takes_lists(3, 1, 1) and not mp.takes_lists(26, 1, 1)      # pairwise: 2 n operands
    assert mp.takes_lists(6, mp.GS_ALL, 2) and mp.takes_lists(5, mp.GS_ALL, 2) and mp.takes_lists(6, mp.GS_ALL, 3)
    assert not mp.takes_lists(1, mp.GS_ALL, 1) and not mp.takes_lists(2, mp.GS_ALL, 2) and mp.takes_lists(4, mp.GS_ALL, 2)
    assert mp.takes_lists(8, 4, 2) and mp.takes_lists(720, 80, 8)      # the groups of he355_bfv_multiply_relin_accumulate
    assert not mp.takes_lists(7, 4, 2) and not mp.takes_lists(8, 4, 3)  # an incomplete group, a ragged row inside a group


def test_lists_or_per_pair_equals_the_header():
    """mp.takes_lists and the sizes it is made of against csrc/behz_lists.h (tests/csim/sim_rules.cpp): every call of the case table at its
    own level, base size and ring, and the batches of test_lists_or_per_pair.  An Indexer3 as to_ix3 (device_types.h) and
    he355_bfv_multiply_relin_accumulate make it: the strides do not enter the decision."""
    import csim_lib
    S = csim_lib.load()
    u64p = C.POINTER(C.c_uint64)
    S.sim_behz_lists.argtypes = [u64p, C.c_uint64, C.c_int, C.c_size_t, C.c_size_t, u64p]

    def header(n, gs, b1, L, S_, N):
        ix = (0, 0, 1, 1, 1, 0, 1, 0) if (gs, b1) == (1, 1) else (0, 0, gs, b1, 0, 1, 0, 1) if gs == mp.GS_ALL else (0, 0, gs, b1, gs // b1, 1, b1, 1)
        out = (C.c_uint64 * 11)()
        S.sim_behz_lists((C.c_uint64 * 8)(*ix), n, L, S_, N, out)
        return dict(zip(("G", "I", "J", "na", "n_cts", "may_list", "e_words", "per_res", "per_op", "a_cts", "b_cts"), (int(v) for v in out)))

    def check(n, gs, b1, L, S_, N):
        g = header(n, gs, b1, L, S_, N)
        assert (g["na"], g["n_cts"]) == (g["G"] * g["I"], g["G"] * (g["I"] + g["J"])), (n, gs, b1)  # (G, I, J themselves: test_behz_sim_cpu.py)
        assert bool(g["may_list"]) == mp.takes_lists(n, gs, b1), (n, gs, b1)
        assert g["e_words"] == g["n_cts"] * 2 * (L + S_) * N and g["per_res"] == 3 * (L + S_) * N and g["per_op"] == 7 * (L + S_) * N
        return g

    took = set()
    for name, L, case in mp.case_table():
        lv = mp.chain_levels(name)[L]
        g = check(case.n, *mp.indexer(case.kind, case.b1), L, lv.S, lv.N)
        took.add(bool(g["may_list"]))
        # the spans the overlap check reads: the last operand of each side, from base 0
        assert (g["a_cts"], g["b_cts"]) == ((case.n, case.n) if case.kind == "pairwise" else (g["I"], g["J"])), case
    assert took == {True, False}
    for n, gs, b1 in [(1, 1, 1), (3, 1, 1), (26, 1, 1), (6, mp.GS_ALL, 2), (5, mp.GS_ALL, 2), (6, mp.GS_ALL, 3), (1, mp.GS_ALL, 1), (2, mp.GS_ALL, 2),
                      (4, mp.GS_ALL, 2), (8, 4, 2), (720, 80, 8), (7, 4, 2), (8, 4, 3)]:
        check(n, gs, b1, 2, 3, 8192)


def test_plans_of_single_calls():
    lv = level(8192, [60, 40, 60], 20, 2)
    zero = dict.fromkeys(mp.COUNTERS, 0)
    assert mp.plan(lv, 6, mp.GS_ALL, 2) == {**zero, "calls_lists": 1, "chunks": 1, "cols_fused": 2, "cols_exact": 2, "inv_dual": 1}
    assert mp.plan(lv, 6, mp.GS_ALL, 3, chunk=4) == {**zero, "calls_lists": 1, "chunks": 2, "cols_fused": 3, "cols_exact": 3, "inv_dual": 2}
    assert mp.plan(lv, 3, 1, 1, chunk=2) == {**zero, "calls_pairs": 1, "chunks": 2, "cols_fused": 4, "cols_exact": 4, "rows_dual": 2}
    assert mp.plan(lv, 26, 1, 1) == {**zero, "calls_pairs": 1, "chunks": 1, "cols_fused": 2, "cols_exact": 2, "rows_split": 1}
    assert mp.plan(lv, 52, 1, 1, chunk=26)["rows_split"] == 2 and mp.plan(lv, 51, 1, 1, chunk=26)["rows_dual"] == 1
    wide = level(8192, [60, 40, 40, 40, 40, 60], 20, 5)
    assert mp.plan(wide, 3, 1, 1) == {**zero, "calls_pairs": 1, "chunks": 1, "cols_unfused": 2, "coef_wide": 2, "rows_dual": 1}
    assert mp.plan(lv, 0, 1, 1) == zero


def test_the_case_table_takes_every_outcome_and_every_instantiation():
    table = mp.case_table()
    seen = set()
    per_level = {}
    for name, L, case in table:
        lv = mp.chain_levels(name)[L]
        out = mp.outcomes(lv, case.n, *mp.indexer(case.kind, case.b1), case.chunk)
        seen |= out
        per_level.setdefault((name, L), set()).update(out)
    want = {"lists", "pairs", "one_chunk", "chunked", "rows_dual", "rows_split", "inv_dual", "inv_split"}
    want |= {"fused" + i for i in mp.FUSED} | {"unfused" + i for i in mp.UNFUSED}
    assert seen == want, seen ^ want
    for (name, L), out in per_level.items():  # every (chain, level) runs both paths, chunked and not
        assert {"lists", "pairs", "one_chunk", "chunked"} <= out, (name, L)
    # both sides of both rules, with the batch sizes read from the launchers, where the issue set them
    for name, L, sizes in (("n8192_default", 2, {"rows_dual": 25, "rows_split": 26, "inv_dual": 34, "inv_split": 35}),
                           ("n16384_d3", 3, {"rows_dual": 9, "rows_split": 10, "inv_dual": 12, "inv_split": 13}),
                           # the split sides closest to the constant: 43 x 3 x 8 = 1032 and 57 x (12 + 6) = 1026 blocks
                           ("n8192_shoup", 1, {"rows_dual": 42, "rows_split": 43, "inv_dual": 56, "inv_split": 57}),
                           # the Shoup build at LOGN1 = 4: two residues on the u64 engine, 9 x 7 x 16 = 1008 and 12 x (60 + 24) = 1008 blocks
                           ("n16384_shoup", 3, {"rows_dual": 9, "rows_split": 10, "inv_dual": 12, "inv_split": 13})):
        got = {c.name.rsplit("_", 1)[0]: c.n for n_, L_, c in table if (n_, L_) == (name, L) and c.name.startswith(("rows_", "inv_"))}
        assert got == sizes, (name, got)
        lv = mp.chain_levels(name)[L]
        for c in (c for n_, L_, c in table if (n_, L_) == (name, L) and c.name.startswith(("rows_", "inv_"))):
            assert mp.outcomes(lv, c.n, *mp.indexer(c.kind, c.b1), c.chunk) >= {c.name.rsplit("_", 1)[0], "one_chunk"}, c
    # the routes the issue's table names, level by level
    inst = {(n, L): mp.instantiation(mp.chain_levels(n)[L]) for n, L in per_level}
    assert inst["n2048", 2] == "<1,4,6,false>" and inst["n4096_d3", 3] == inst["n4096_d3", 1] == "<2,4,6,false>"
    assert [inst["n8192_d4", L] for L in (4, 3, 2, 1)] == ["<3,4,4,true>", "<3,3,3,true>", "<3,2,2,true>", "<3,4,6,false>"]
    assert inst["n8192_d5", 5] == "<16,24>" and inst["n8192_d5", 4] == "<3,4,4,true>"
    assert inst["n8192_60x4", 4] == inst["n8192_60x4", 2] == "<3,4,6,false>"
    assert all(inst[k] == "<4,4,6,false>" for k in inst if k[0].startswith("n16384"))
    assert all(inst[k] == "<4,6>" for k in inst if k[0] in ("n32768_d3", "n32768_shoup", "n1024"))
    # the Shoup build at N >= 16384: the same instantiations as the fold chains of the same length -- other machine code -- with the
    # 60- and the 50-bit data prime on the u64 engine, the 40-bit one and the whole auxiliary base on the fp64 engine
    assert {k for k in inst if k[0] in mp.SHOUP_RINGS} == {("n16384_shoup", 3), ("n16384_shoup", 1), ("n32768_shoup", 3)}
    s16, s32 = mp.chain_levels("n16384_shoup"), mp.chain_levels("n32768_shoup")
    assert (s16[3].nB, s16[3].n_f, s16[3].n_u, s16[3].lds_bytes) == (3, 5, 2, 56 * KIB) and s16[3].fp64[:3] == (False, False, True)
    assert (s16[1].nB, s16[1].n_f, s16[1].n_u, s16[1].lds_bytes) == (2, 3, 1, 32 * KIB)
    assert (s32[3].nB, s32[3].n_f, s32[3].n_u) == (4, 6, 2) and s32[3].fp64[:3] == (False, False, True)
    import shoup_rings as sr
    for name, ring in mp.SHOUP_RINGS.items():
        assert mp.CHAINS[name][0] == (sr.RINGS[ring]["N"], sr.RINGS[ring]["bits"], sr.PLAIN_BITS) and not mp.CHAINS[name][1], name
    x = mp.chain_levels("n8192_60x4")
    assert x[4].fp64[:4] == (False,) * 4 and x[2].fp64[:2] == (False,) * 2  # every data prime on the u64 engine
    assert not any(mp.chain_levels("n8192_force_u64")[2].fp64)
    # few enough products for the oracle: no case above 60, the whole table a few thousand
    assert max(c.n for _, _, c in table) <= 60


def test_the_stats_call_is_exported_declared_and_bound():
    be = importlib.import_module("reference-seal-backend_amd")
    lib = C.CDLL(be.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "he355.h")).read()
    s = "he355_bfv_multiply_stats"
    assert hasattr(lib, s) and s in be.C_ABI_SYMBOLS and (s + "(") in hdr and hasattr(be.Context, "bfv_multiply_stats")
    body = re.search(r"typedef struct \{([^}]*)\} he355_bfv_multiply_stats_t;", hdr).group(1)
    fields = re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [k for k, _ in be.BfvMultiplyStats._fields_] == list(mp.COUNTERS) + ["lds_limit", "reserved"]
    assert C.sizeof(be.BfvMultiplyStats) == 16 * 8
    # he355_bfv_route_stats_t stays as it was: eleven counters and five reserved words
    assert C.sizeof(be.BfvRouteStats) == 16 * 8 and be.BfvRouteStats._fields_[-1][0] == "reserved"
    ctx = be.Context(be.SCHEME_BFV, 4096, bit_sizes=[60, 40, 40, 60], plain_bits=20, sec128=False)  # no device: the call fails loudly
    with pytest.raises(be.HE355Error):
        ctx.bfv_multiply_stats()
    assert be.lib().he355_bfv_multiply_stats(ctx.h, None, 0) != 0
