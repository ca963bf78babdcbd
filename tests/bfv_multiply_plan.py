"""The host-side kernel selection of the BEHZ multiply (`behz_lists` in csrc/behz_lists.h and `bfv_multiply3` in csrc/he355_api.hip, the
`launch_behz_*` functions and `behz_cols_fusable` in csrc/he355_kernels_behz.hip) restated in plain Python, in the manner of tests/launch_plan.py:
it restates the rules, it does not link them (tests/test_bfv_multiply_plan_cpu.py holds `takes_lists` to the header).  Tests use it to (a) derive the batches that lie on both sides of every decision instead of guessing them and (b) assert
the counters of `he355_bfv_multiply_stats` against a plan.  When the restatement and the product disagree, the product decides and this
file is what gets corrected.

The auxiliary base of a level (its size nB and its primes) and the chain's primes come from the CPU build of the product's parameter code
(tests/csim, `sim_behz_base`), never from the device library; a residue runs on the fp64 engine when its prime is below 2^47 and
HE355_FORCE_U64 is not 1 (Params::Params).

The decisions of one call at level L, n results, indexer (gs, b1), chunk c:

1. lists or per-pair: `lists = (G == 1 or (n % gs == 0 and gs % b1 == 0)) and n_cts <= n`, n_cts the distinct operands;
2. fused or unfused column passes: `L <= 4 and nB <= 6 and 1 <= logn1 <= 4 and (L + nB + 1) * (64 << logn1) * 8 <= lds_limit`, lds_limit what the
   device grants one block (he355_bfv_multiply_stats reports it); the fused pair comes in seven instantiations, the unfused coefficient kernels in two;
3. per chunk of n_c results, one launch for both engines or one per engine: per-pair `n_c (L + S) 2^logn1 <= 1024`, lists
   `ceil(3 n_c n_f 2^logn1 / 4) + ceil(3 n_c n_u 2^logn1 / 4) <= 1024` (S = nB + 1; n_f / n_u residues of q and Bsk on the fp64 / u64 engine), and
   only where both engines have residues;
4. the chunk: min(c, n) results at a time (the halving when the arena does not fit is not restated: the tests stay far below it).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass

K_WAVES = 4                      # kernel_common.inc
DUAL_MAX_BLOCKS = 1024           # ks_launch.h: kDualMaxBlocks
DEFAULT_CHUNK = 1024             # ks_shape.h: KsLimits::chunk
LDS_NO_OPT_IN = 64 << 10         # what every HIP device grants a block without asking
LDS_MI355X = 160 << 10           # CDNA4: the LDS of one CU, all of which one workgroup may take
GS_ALL = 2 ** 64 - 1             # Indexer3::gs of an outer product (one group)
COUNTERS = ("calls_lists", "calls_pairs", "chunks", "cols_fused", "cols_unfused", "cols_exact", "coef_wide", "rows_dual", "rows_split",
            "inv_dual", "inv_split")
FUSED = ("<1,4,6,false>", "<2,4,6,false>", "<4,4,6,false>", "<3,2,2,true>", "<3,3,3,true>", "<3,4,4,true>", "<3,4,6,false>")
UNFUSED = ("<4,6>", "<16,24>")


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


@dataclass(frozen=True)
class Level:
    """one level of a chain: ring degree, data primes, auxiliary base size, the engine of every residue of q then Bsk (True: fp64)"""
    N: int
    L: int
    nB: int
    fp64: tuple

    @property
    def logn1(self):
        return self.N.bit_length() - 1 - 10

    @property
    def S(self):
        return self.nB + 1

    @property
    def n_f(self):
        return sum(self.fp64)

    @property
    def n_u(self):
        return len(self.fp64) - self.n_f

    @property
    def lds_bytes(self):
        return (self.L + self.nB + 1) * (64 << self.logn1) * 8


@functools.lru_cache(maxsize=None)
def _sim():
    import csim_lib
    lib = csim_lib.load()
    u64p = C.POINTER(C.c_uint64)
    lib.sim_behz_create.restype = C.c_void_p
    lib.sim_behz_create.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int]
    lib.sim_behz_destroy.argtypes = [C.c_void_p]
    lib.sim_behz_levels.restype = C.c_size_t
    lib.sim_behz_levels.argtypes = [C.c_void_p]
    lib.sim_behz_q.restype = C.c_uint64
    lib.sim_behz_q.argtypes = [C.c_void_p, C.c_size_t]
    lib.sim_behz_base.restype = C.c_size_t
    lib.sim_behz_base.argtypes = [C.c_void_p, C.c_int, u64p]
    return lib


@functools.lru_cache(maxsize=None)
def levels(N: int, bits: tuple, plain_bits: int, force_u64: bool = False, seal_base: bool = False) -> dict:
    """{L: Level} of every level of the chain, the environment set as the device context's would be"""
    sim = _sim()
    saved = {k: os.environ.get(k) for k in ("HE355_FORCE_U64", "HE355_BEHZ_BASE")}
    try:
        for k, on, v in (("HE355_FORCE_U64", force_u64, "1"), ("HE355_BEHZ_BASE", seal_base, "seal")):
            if on:
                os.environ[k] = v
            else:
                os.environ.pop(k, None)
        h = sim.sim_behz_create(N, (C.c_int * len(bits))(*bits), len(bits), plain_bits)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert h, (N, bits, plain_bits)
    try:
        out = {}
        for L in range(1, int(sim.sim_behz_levels(h)) + 1):
            buf = (C.c_uint64 * 64)()
            S = int(sim.sim_behz_base(h, L, buf))  # m_sk, B_0, ..
            primes = [int(sim.sim_behz_q(h, i)) for i in range(L)] + [int(buf[i]) for i in range(1, S)] + [int(buf[0])]
            out[L] = Level(N, L, S - 1, tuple((not force_u64) and q < 2 ** 47 for q in primes))
        return out
    finally:
        sim.sim_behz_destroy(h)


# ---- decision 1: the distinct-operand lists (behz_lists.h) ------------------------------------------------------------------------------
def indexer(kind: str, b1: int = 1):
    """(gs, b1) of Context.pairwise() / Context.outer(.., b1) after to_ix3 (device_types.h)"""
    return (1, 1) if kind == "pairwise" else (GS_ALL, b1)


def takes_lists(n: int, gs: int, b1: int) -> bool:
    gsz = min(gs, n)
    G = 1 if gs >= n else _cdiv(n, gs)
    I, J = _cdiv(gsz, b1), min(b1, gsz)
    n_cts = G * I + G * J
    return (G == 1 or (n % gs == 0 and gs % b1 == 0)) and n_cts <= n


# ---- decision 2: the column passes (behz_cols_fusable, the two launchers' switches) ----------------------------------------------------------
def fusable(lv: Level, lds_limit: int = LDS_MI355X) -> bool:
    return lv.L <= 4 and lv.nB <= 6 and 1 <= lv.logn1 <= 4 and lv.lds_bytes <= lds_limit


def instantiation(lv: Level, lds_limit: int = LDS_MI355X) -> str:
    """the template arguments of the column kernels this level runs: k_behz_extend_cols / k_behz_cols_floor_sk<LOGN1, ML, MB, EXACT>, or
    k_behz_extend / k_behz_floor_sk<ML, MB>"""
    if not fusable(lv, lds_limit):
        return "<4,6>" if lv.L <= 4 and lv.nB <= 6 else "<16,24>"
    if lv.logn1 != 3:
        return f"<{lv.logn1},4,6,false>"
    if lv.L == lv.nB and 2 <= lv.L <= 4:
        return f"<3,{lv.L},{lv.L},true>"
    return "<3,4,6,false>"


# ---- decision 3: one launch for both engines ---------------------------------------------------------------------------------------------
def rows_dual(lv: Level, n_c: int) -> bool:
    ge = [(n_c * r) << lv.logn1 for r in (lv.n_f, lv.n_u)]
    return bool(ge[0] and ge[1] and ge[0] + ge[1] <= DUAL_MAX_BLOCKS)


def inv_dual(lv: Level, n_c: int) -> bool:
    jobs = [((n_c * r) << lv.logn1) * 3 for r in (lv.n_f, lv.n_u)]
    return bool(jobs[0] and jobs[1] and _cdiv(jobs[0], K_WAVES) + _cdiv(jobs[1], K_WAVES) <= DUAL_MAX_BLOCKS)


# ---- one call -----------------------------------------------------------------------------------------------------------------------------
def plan(lv: Level, n: int, gs: int, b1: int, chunk: int = DEFAULT_CHUNK, lds_limit: int = LDS_MI355X) -> dict:
    """the counters he355_bfv_multiply_stats shows after one he355_bfv_multiply of n results (those at zero included)"""
    p = dict.fromkeys(COUNTERS, 0)
    if not n:
        return p
    c = min(chunk if chunk else 1, n)
    sizes = [min(c, n - off) for off in range(0, n, c)]
    lists = takes_lists(n, gs, b1)
    p["calls_lists" if lists else "calls_pairs"] = 1
    p["chunks"] = len(sizes)
    cols = 1 + len(sizes) if lists else 2 * len(sizes)  # extensions + floor steps
    inst = instantiation(lv, lds_limit)
    if fusable(lv, lds_limit):
        p["cols_fused"] = cols
        p["cols_exact"] = cols if inst.endswith("true>") else 0
    else:
        p["cols_unfused"] = cols
        p["coef_wide"] = cols if inst == "<16,24>" else 0
    for n_c in sizes:
        if lists:
            p["inv_dual" if inv_dual(lv, n_c) else "inv_split"] += 1
        else:
            p["rows_dual" if rows_dual(lv, n_c) else "rows_split"] += 1
    return p


def outcomes(lv: Level, n: int, gs: int, b1: int, chunk: int = DEFAULT_CHUNK, lds_limit: int = LDS_MI355X) -> set:
    """the decision outcomes one call takes, as names: path, column route + instantiation, the dual / split launches, chunked or not"""
    p = plan(lv, n, gs, b1, chunk, lds_limit)
    out = {"lists" if p["calls_lists"] else "pairs", ("fused" if p["cols_fused"] else "unfused") + instantiation(lv, lds_limit),
           "one_chunk" if p["chunks"] == 1 else "chunked"}
    out |= {k for k in ("rows_dual", "rows_split", "inv_dual", "inv_split") if p[k]}
    return out


@dataclass(frozen=True)
class Case:
    name: str
    kind: str   # "pairwise" or "outer"
    n: int
    b1: int
    chunk: int


def _threshold(dual, hi=4096):
    """the largest n_c the rule sends to the dual launch (None: never dual, one engine has no residue)"""
    if not dual(1):
        return None
    n_c = 1
    while n_c < hi and dual(n_c + 1):
        n_c += 1
    return n_c


def thresholds(lv: Level) -> dict:
    """{"rows": (dual at, split at) or None, "inv": ...}: the chunk sizes on both sides of the two 1024-block rules"""
    r, i = _threshold(lambda k: rows_dual(lv, k)), _threshold(lambda k: inv_dual(lv, k))
    return {"rows": None if r is None else (r, r + 1), "inv": None if i is None else (i, i + 1)}


def _outer_b1(n: int) -> int:
    """the row length of a (possibly ragged) outer product of n results that takes the lists path with the fewest operands"""
    best = min(range(1, n + 1), key=lambda b: (_cdiv(n, b) + min(b, n), b))
    assert takes_lists(n, GS_ALL, best), n
    return best


def boundary_cases(lv: Level, with_thresholds: bool = False) -> list:
    """the smallest calls on both sides of every decision of one level: the five call shapes every (chain, level) runs and, with_thresholds,
    the four batches at the two 1024-block rules (none where one engine has every residue)"""
    cases = [
        Case("outer_3x2", "outer", 6, 2, DEFAULT_CHUNK),           # lists
        Case("outer_ragged_5", "outer", 5, 2, DEFAULT_CHUNK),      # lists, the last row incomplete
        Case("pairwise_3", "pairwise", 3, 1, DEFAULT_CHUNK),       # per-pair
        Case("single", "pairwise", 1, 1, DEFAULT_CHUNK),           # per-pair, n = 1
        Case("outer_2x3_chunk4", "outer", 6, 3, 4),                # lists, chunks of 4 and 2: the first ends inside row 1
        Case("pairwise_3_chunk2", "pairwise", 3, 1, 2),            # per-pair, chunks of 2 and 1
    ]
    for c in cases:
        assert takes_lists(c.n, *indexer(c.kind, c.b1)) == (c.kind == "outer"), c
    if with_thresholds:
        th = thresholds(lv)
        if th["rows"]:
            cases += [Case(f"rows_dual_{th['rows'][0]}", "pairwise", th["rows"][0], 1, DEFAULT_CHUNK),
                      Case(f"rows_split_{th['rows'][1]}", "pairwise", th["rows"][1], 1, DEFAULT_CHUNK)]
        if th["inv"]:
            cases += [Case(f"inv_dual_{th['inv'][0]}", "outer", th["inv"][0], _outer_b1(th["inv"][0]), DEFAULT_CHUNK),
                      Case(f"inv_split_{th['inv'][1]}", "outer", th["inv"][1], _outer_b1(th["inv"][1]), DEFAULT_CHUNK)]
    return cases


# ---- the case table of tests/test_gpu_bfv_multiply_routes.py -------------------------------------------------------------------------------
# name: ((N, key-level bit sizes, plain bits), force_u64, seal_base, levels run, levels that also run the threshold batches)
CHAINS = {
    "n2048": ((2048, (60, 40, 60), 20), False, False, (2,), ()),
    "n4096_d3": ((4096, (60, 40, 40, 60), 20), False, False, (3, 1), ()),
    "n8192_d4": ((8192, (60, 40, 40, 40, 60), 20), False, False, (4, 3, 2, 1), ()),
    "n8192_d5": ((8192, (60, 40, 40, 40, 40, 60), 20), False, False, (5, 4), ()),
    "n8192_60x4": ((8192, (60, 60, 60, 60, 60), 20), False, False, (4, 2), ()),
    # L = 1 also runs the threshold batches: its block counts step by 24 and 18 per result, 43 x 24 = 1032 and 57 x 18 = 1026 lie just above 1024
    "n8192_shoup": ((8192, (50, 40, 50), 20), False, False, (2, 1), (1,)),
    "n8192_default": ((8192, (60, 40, 60), 20), False, False, (2,), (2,)),
    "n8192_force_u64": ((8192, (60, 40, 60), 20), True, False, (2,), ()),
    "n8192_seal_base": ((8192, (60, 40, 60), 20), False, True, (2,), ()),
    "n16384_d3": ((16384, (60, 40, 40, 60), 20), False, False, (3, 2, 1), (3,)),
    "n16384_d4": ((16384, (60, 40, 40, 40, 60), 20), False, False, (4,), ()),
    "n16384_60x4": ((16384, (60, 60, 60, 60, 60), 31), False, False, (3, 4), ()),
    "n32768_d3": ((32768, (60, 40, 40, 60), 20), False, False, (3, 1), ()),
    "n1024": ((1024, (50, 40, 50), 20), False, False, (2, 1), ()),
    # the Shoup build of the u64 engine at LOGN1 = 4 and 5 (the chains of tests/shoup_rings.py: a 60- and a 50-bit prime on that engine)
    "n16384_shoup": ((16384, (60, 50, 40, 60), 20), False, False, (3, 1), (3,)),
    "n32768_shoup": ((32768, (60, 50, 40, 60), 20), False, False, (3,), ()),
}
SHOUP_RINGS = {"n16384_shoup": "n16384_60_50_40_60_shoup", "n32768_shoup": "n32768_60_50_40_60_shoup"}  # chain: its entry of shoup_rings.RINGS


def chain_levels(name: str) -> dict:
    (N, bits, pb), force, seal, _, _ = CHAINS[name]
    return levels(N, tuple(bits), pb, force, seal)


def case_table() -> list:
    """[(chain, L, Case)]: every call the GPU module makes"""
    rows = []
    for name, (_, _, _, run, thr) in CHAINS.items():
        lv = chain_levels(name)
        for L in run:
            rows += [(name, L, c) for c in boundary_cases(lv[L], L in thr)]
    return rows
