"""The library's kernel-selection rules restated in plain Python (a helper module: no GPU, no ctypes, nothing compiled).

A key switch is never "the key switch": per chunk the library picks a kernel sequence (`ks_shape`, csrc/ks_shape.h) and per launch a
grid (csrc/ks_launch.h, which `launch_k1`, `launch_k2`, `launch_k3`, `launch_k3_combine`, `launch_floor_cols`, `launch_floor_rows` and
`launch_rows_inv_select` of csrc/he355_kernels_ks.hip, he355_kernels_k3.hip and he355_kernels.hip call; the ring-in-LDS launchers of csrc/he355_kernels_lds.hip hold theirs) from the
batch, the ring, the level and the engine of each prime.  This module restates those rules -- it does not link them
(tests/test_launch_plan_cpu.py holds the shape rule to csrc/ks_shape.h and every `plan_*` launcher function to csrc/ks_launch.h on the
CPU; the three grids of the LDS shape in `plan_chunk` are literals) -- so that tests can (a) derive the batch sizes that lie on both sides of every threshold instead of guessing them,
(b) assert the path counters of `he355_path_stats` against a plan, and (c) compare a kernel trace with the planned launches
(tools/plan_vs_trace.py).  When the restatement and the product disagree, the product decides and this file is what gets corrected.

A *plan* of one call is a `CallPlan`: the chunks in issue order, each with its shape and its launches (kernel family, grid in blocks,
threads per block, op-groups per block, waves, target split), and the call's path counters.

What is not restated: the coefficient-form BFV key switch (`KsShape::BfvCoeff`: one shape, no counter -- its chunks carry no launches
here), the halving of a chunk when the scratch arenas do not fit the device (the tests stay far below that), and kernels that are not
part of a key switch (copies, additions, the NTTs around a BFV rotation chain).
"""
from __future__ import annotations

from dataclasses import dataclass, field

K_WAVES, K_BLOCK = 4, 256                      # ks_launch.h: kWaves, kBlock
DUAL_MAX_BLOCKS, DUAL_MAX_BLOCKS_K3 = 1024, 4096  # ks_launch.h: kDualMaxBlocks, kDualMaxBlocksK3
LAT_TARGETS, LAT_SPLIT, LAT_SPLIT_U64 = 8, 2, 8   # ks_shape.h: kLatTargets, kLatSplit, kLatSplitU64
DEFAULT_CHUNK = 1024
SCAN_MAX = 512                                 # the largest batch boundary_cases looks at


def _cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


@dataclass(frozen=True)
class Chain:
    """scheme "ckks" / "bfv", ring degree, key-level bit sizes (special prime last) and the engine of each prime (True: fp64 engine) --
    `Context.fp64` where a device context exists, else `engines(bits)`"""
    scheme: str
    N: int
    bits: tuple
    fp64: tuple

    @property
    def K(self):
        return len(self.bits)

    @property
    def Ltop(self):
        return max(1, self.K - 1)

    @property
    def logn1(self):
        return self.N.bit_length() - 1 - 10


def engines(bits) -> tuple:
    """Params::Params: a prime below 2^47 runs on the fp64 engine, every other one on the u64 engine"""
    return tuple(b <= 47 for b in bits)


def chain(scheme: str, N: int, bits, fp64=None) -> Chain:
    return Chain(scheme, N, tuple(bits), tuple(bool(x) for x in fp64) if fp64 is not None else engines(bits))


# ---- the shape rule (ks_shape.h; tests/test_launch_plan_cpu.py holds each function to it) ----------------------------------------------
def lat_limit(ch: Chain) -> int:
    return min(12, max(1, (1 << 17) // ch.N))


def latency_shape(ch: Chain, nc: int, ntt_pipeline: bool = True) -> bool:
    """ntt_pipeline False: asked of a BFV context's own environment (rotate_sum's node-by-node test), which has no latency shape"""
    return (ch.scheme == "ckks" or ntt_pipeline) and nc <= lat_limit(ch) and ch.K >= 2


def lds_supported(ch: Chain, L: int) -> bool:
    return 0 <= ch.logn1 <= 3 and 1 <= L <= 6 and ch.K >= 2 and L <= ch.K - 1


def lds_limit(ch: Chain, L: int) -> int:
    blocks = 384 << (3 - min(3, ch.logn1))
    return max(1, blocks // ((L + 1) * L))


def lds_shape(ch: Chain, L: int, nc: int) -> bool:
    return lds_supported(ch, L) and nc <= lds_limit(ch, L)


def k3_can_fuse(ch: Chain) -> bool:
    return ch.K >= 2  # (on the NTT-domain pipeline, which is where every planned launch runs)


def fuse_pays(ch: Chain, nc: int, L: int) -> bool:
    sp_blocks = (1 << ch.logn1) * _cdiv(nc, 8)
    return sp_blocks >= 128 or sp_blocks * L >= 1536


def level_sum_pays(ch: Chain, L: int, n: int, chunk: int = DEFAULT_CHUNK) -> bool:
    if n % 8 or not k3_can_fuse(ch) or not fuse_pays(ch, n, L) or chunk < n:
        return False
    return ((L << ch.logn1) * (n // 8)) >= 512


def ks_shape(ch: Chain, L: int, nc: int, kind: str, out_apart: bool, coeff: bool = False) -> str:
    """kind: "product", "size3", "galois", "grouped"; coeff: a BFV context's coefficient-form ciphertexts"""
    if coeff:
        return "bfv_coeff"
    if kind != "grouped" and out_apart and lds_shape(ch, L, nc):
        return "lds"
    if kind != "grouped" and latency_shape(ch, nc):
        return "latency"
    return "fused" if k3_can_fuse(ch) and fuse_pays(ch, nc, L) else "unfused"


# ---- launches -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    family: str          # kernel name without its template arguments
    grid: tuple          # blocks (x, y)
    block: int           # threads per block
    og_per_block: int = 0
    waves: int = 0
    ts: int = 0
    engine: str = ""     # "fp64", "u64", "both" or ""
    note: str = ""

    def key(self):
        return (self.family, self.grid[0], self.grid[1], self.block)


def plan_k1(ch: Chain, L: int, mode: str, n: int, no_c01: bool) -> list:
    gp, ni = [0, 0], [0, 0]
    for p in range(2):
        ni[p] = sum(1 for i in range(L) if ch.fp64[i] == (p == 0))
        gp[p] = _cdiv((n * ni[p]) << ch.logn1, K_WAVES) if ni[p] else 0
    if gp[0] and gp[1] and (n <= 8 or gp[0] + gp[1] <= DUAL_MAX_BLOCKS) and not (mode == "product" and no_c01):
        return [Launch("k_k1_dual", (gp[0] + gp[1], 1), K_BLOCK, engine="both")]
    return [Launch("k_k1", ((ni[p] << ch.logn1) * _cdiv(n, K_WAVES), 1), K_BLOCK, engine="fp64" if p == 0 else "u64") for p in range(2) if gp[p]]


def _target_split(gw: int, n_tgt: int, tsplit: int) -> int:
    if tsplit > 1:
        return tsplit

    def cost(c):
        return float(_cdiv(gw * c, 512)) * (1.0 + 1.2 * _cdiv(n_tgt, c))
    c1 = best = cost(1)
    ts = 1
    for c in (2, 4):
        if cost(c) < best * 0.95 and cost(c) < c1 * 0.95:
            best, ts = cost(c), c
    return ts


def plan_k2(ch: Chain, L: int, n: int, tsplit: int = 1) -> list:
    n_tgt = L  # L + 1 targets less the digit's own prime on the NTT-domain pipeline
    gk = [0, 0]
    for wide in range(2):
        gk[wide] = n * sum(1 for j in range(L) if (ch.bits[j] >= 53) == bool(wide)) * 4
    if gk[0] and gk[1]:
        ts = _target_split(gk[0] + gk[1], n_tgt, tsplit)
        if tsplit > 1 or (gk[0] + gk[1]) * ts <= DUAL_MAX_BLOCKS:
            return [Launch("k_k2n_dual", (gk[0] + gk[1], ts), K_BLOCK, ts=ts, engine="both")]
    out = []
    for wide in range(2):
        if gk[wide]:
            ts = _target_split(gk[wide], n_tgt, tsplit)
            out.append(Launch("k_k2n", (gk[wide], ts), K_BLOCK, ts=ts, note="60-bit digits" if wide else "digits below 2^52"))
    return out


def _size_grid(tiles: int, n_ops: int, w: int, u64_pass: bool, L: int):
    """ks_launch.h, k3_size_grid: (op-groups, op-groups per block, blocks)"""
    n_og = _cdiv(n_ops, w)
    og_max = (4 if n_og >= 128 else 2) if w == 8 else 4
    work = (14.0 if u64_pass else 7.0) * (L + 2) * (0.5 if w == 4 else 1.0)
    startup = 4.0
    ogpb, best = og_max, 0.0
    c = og_max
    while c >= 1:
        blocks = tiles * _cdiv(n_og, c)
        cost = float(_cdiv(blocks, 256)) * (c * work + startup)
        if c == og_max or cost < best * 0.999:
            best, ogpb = cost, c
        c >>= 1
    return n_og, ogpb, _cdiv(tiles, 8) * 8 * _cdiv(n_og, ogpb)


def plan_k3(ch: Chain, L: int, n: int, part: str, fuse: bool = False, tt_lo: int = 0, tt_hi: int | None = None, n_split: int = 1,
            n_split_u64: int = 0, group_size: int = 0, level_sum: bool = False, note: str = "") -> list:
    """part: "all", "special", "data"; fuse: the mod-down in the epilogue, data primes tt_lo <= tt < tt_hi; n_split > 1: the latency shape;
    group_size > 0: a grouped launch, level_sum: with KsGroups::sum_out"""
    if n_split_u64 <= 0:
        n_split_u64 = n_split
    pend = []
    for p in range(2):
        n_tt = 0
        for tt in range(L + 1):
            if (part == "special" and tt != L) or (part == "data" and tt == L):
                continue
            if fuse and (tt < tt_lo or tt >= (L if tt_hi is None else tt_hi)):
                continue
            t = ch.K - 1 if tt == L else tt
            n_tt += ch.fp64[t] == (p == 0)
        if not n_tt:
            continue
        split = (n_split if p == 0 else n_split_u64) if n_split > 1 else 1
        waves = 1 if split > 1 else 8
        tiles = n_tt << ch.logn1
        n_og, ogpb, g = _size_grid(tiles, n, waves, p == 1, L)
        sums = bool(group_size) and level_sum and fuse
        if sums:
            gs8 = group_size // 8
            assert waves == 8 and group_size % 8 == 0 and n % group_size == 0
            ogpb, g = n_og // gs8, _cdiv(tiles, 8) * 8 * gs8
        if p == 1 and waves == 8 and g <= 128 and not sums:
            n_og4, ogpb4, g4 = _size_grid(tiles, n, 4, True, L)
            if g4 + (pend[0]["g"] if pend else 0) <= 256:
                waves, n_og, ogpb, g = 4, n_og4, ogpb4, g4
        pend.append(dict(g=g, f64=p == 0, waves=waves, ogpb=ogpb, split=split, sums=sums))
    if not pend:
        return []
    if len(pend) == 2 and pend[0]["waves"] == 1:
        return [Launch("k_k3_dual", (pend[0]["g"] + pend[1]["g"], max(pend[0]["split"], pend[1]["split"])), 64, waves=1, engine="both", note=note)]
    if len(pend) == 2 and pend[0]["waves"] == 8 and pend[0]["g"] + pend[1]["g"] <= DUAL_MAX_BLOCKS_K3:
        return [Launch("k_k3_dual8", (pend[0]["g"] + pend[1]["g"], 1), 512, og_per_block=pend[0]["ogpb"], waves=pend[1]["waves"], engine="both",
                       note=(note + f" og_per_block fp64 {pend[0]['ogpb']} u64 {pend[1]['ogpb']}").strip())]
    return [Launch("k_k3", (q["g"], q["split"]), 64 * q["waves"], og_per_block=q["ogpb"], waves=q["waves"], engine="fp64" if q["f64"] else "u64",
                   note=note) for q in pend]


def plan_k3_combine(ch: Chain, L: int, n: int) -> list:
    return [Launch("k_k3_combine", (_cdiv((n * 2 * (L + 1)) << ch.logn1, K_WAVES), 1), K_BLOCK)]


def plan_floor_cols(ch: Chain, n_polys: int, n_tgt: int, tsplit: int = 1) -> list:
    if not n_polys or n_tgt <= 0:
        return []
    ts = tsplit if tsplit > 1 else 1
    return [Launch("k_floor_colsn", (n_polys * 4, ts), K_BLOCK, ts=ts)]


def plan_floor_rows(ch: Chain, n: int, n_tgt: int, n_src: int, tail_prime: int = -1) -> list:
    n_jobs = n * n_src
    jpb = 8 * K_WAVES
    while jpb > K_WAVES and (((n_tgt << ch.logn1) * _cdiv(n_jobs, jpb)) < 256 * 8 or jpb // 2 >= n_jobs):
        jpb >>= 1
    per = _cdiv(n_jobs, jpb)
    if tail_prime < 0:
        ge = [(sum(1 for i in range(n_tgt) if ch.fp64[i] == (e == 0)) << ch.logn1) * per for e in range(2)]
        if ge[0] and ge[1] and (n <= 8 or ge[0] + ge[1] <= DUAL_MAX_BLOCKS):
            return [Launch("k_floor_rows_dual", (ge[0] + ge[1], 1), K_BLOCK, engine="both")]
    out = []
    for p in range(4):
        f64, tail = p < 2, bool(p & 1)
        ni = sum(1 for i in range(n_tgt) if ch.fp64[i] == f64 and (i == tail_prime) == tail)
        if ni:
            note = "tail prime" if tail else "beside the tail prime's launch" if tail_prime >= 0 else ""
            out.append(Launch("k_floor_rows", ((ni << ch.logn1) * per, 1), K_BLOCK, engine="fp64" if f64 else "u64", note=note))
    return out


def plan_rows_inv_select(ch: Chain, n_polys: int) -> list:
    return [Launch("k_rows_inv_select", (_cdiv(n_polys << ch.logn1, K_WAVES), 1), K_BLOCK)] if n_polys else []


def plan_rescale_tail(ch: Chain, L: int, size: int, nc: int) -> list:
    ls = plan_floor_cols(ch, nc * size, L - 1, LAT_TARGETS if latency_shape(ch, nc) else 1)
    return ls + plan_floor_rows(ch, nc, L - 1, size, -1)


@dataclass
class ChunkPlan:
    off: int
    nc: int
    shape: str
    in_k3: bool = False          # k_k3 forms c0, c1 itself (fused and out_apart)
    level_sum: bool = False      # this launch adds its groups into the level's sum
    stream: int = 0
    launches: list = field(default_factory=list)


def plan_chunk(ch: Chain, L: int, nc: int, kind: str, out_apart: bool, rescale: bool, group_size: int = 0, level_sum: bool = False,
               coeff: bool = False) -> ChunkPlan:
    """one chunk's kernel sequence: key_switch_batch's lambda and key_switch_tail"""
    shape = ks_shape(ch, L, nc, kind, out_apart, coeff)
    cp = ChunkPlan(0, nc, shape)
    ls = cp.launches
    if shape == "bfv_coeff":
        return cp
    n1 = 1 << ch.logn1
    if shape == "lds":
        ls.append(Launch("k_lds_digits", (nc * (L + 1) * L, 1), 64 * n1))
        ls.append(Launch("k_lds_floor", (nc * 2 * L, 1), 64 * n1, note="mod-down"))
        if rescale:
            ls.append(Launch("k_lds_floor", (nc * 2 * (L - 1), 1), 64 * n1, note="rescale"))
        return cp
    fused, lat = shape == "fused", shape == "latency"
    product = kind == "product"
    cp.in_k3 = fused and out_apart
    cp.level_sum = fused and level_sum
    assert not (level_sum and not fused), "level sum: the fused key switch only"
    k1_mode = "product" if product else "galois" if kind in ("galois", "grouped") else "size3"
    ls += plan_k1(ch, L, k1_mode, nc, cp.in_k3 and product)
    ls += plan_k2(ch, L, nc, LAT_TARGETS if lat else 1)
    SP_polys = nc * 2
    gs = group_size if kind == "grouped" else 0
    if lat:
        ls += plan_k3(ch, L, nc, "all", n_split=LAT_SPLIT, n_split_u64=LAT_SPLIT_U64)
        ls += plan_k3_combine(ch, L, nc)
        ls += plan_floor_cols(ch, SP_polys, L, LAT_TARGETS)
    elif not fused:
        ls += plan_k3(ch, L, nc, "all", group_size=gs)
        ls += plan_floor_cols(ch, SP_polys, L)
    else:
        ls += plan_k3(ch, L, nc, "special", group_size=gs, level_sum=cp.level_sum, note="special prime")
        if rescale:
            raw = cp.in_k3 and product
            if raw:
                ls += plan_k3(ch, L, nc, "data", True, L - 1, L, note="divided-out prime, raw tail")
            else:
                ls += plan_floor_cols(ch, SP_polys, 1)
                ls += plan_k3(ch, L, nc, "data", True, L - 1, L, note="divided-out prime")
                ls += plan_rows_inv_select(ch, SP_polys)
            ls += plan_floor_cols(ch, SP_polys, L - 1)
            ls += plan_k3(ch, L, nc, "data", True, 0, L - 1, note="data primes, rescale in the epilogue")
            return cp
        ls += plan_floor_cols(ch, SP_polys, L)
        ls += plan_k3(ch, L, nc, "data", True, 0, L, group_size=gs, level_sum=cp.level_sum, note="data primes")
        return cp
    ls += plan_floor_rows(ch, nc, L, 2, L - 1 if rescale else -1)
    if rescale:
        ls += plan_rescale_tail(ch, L, 2, nc)
    return cp


COUNTERS = ("ks_lds", "ks_latency", "ks_unfused", "ks_fused", "level_sums_in_k3", "level_sums_by_kernel")


@dataclass
class CallPlan:
    op: str
    L: int
    n: int
    out_apart: bool
    chunks: list = field(default_factory=list)
    level_sums_in_k3: int = 0
    level_sums_by_kernel: int = 0
    key_switches: int = 0  # rotate_sum: Galois key switches per ciphertext

    def counters(self) -> dict:
        c = dict.fromkeys(COUNTERS, 0)
        for cp in self.chunks:
            if cp.shape != "bfv_coeff":
                c["ks_" + cp.shape] += 1
        c["level_sums_in_k3"], c["level_sums_by_kernel"] = self.level_sums_in_k3, self.level_sums_by_kernel
        return c

    def launches(self) -> list:
        return [l for cp in self.chunks for l in cp.launches]


def plan_batch(ch: Chain, L: int, n: int, kind: str, out_apart: bool, rescale: bool, chunk: int = DEFAULT_CHUNK, may_dual: bool = False,
               group_size: int = 0, sum_out: bool = False, coeff: bool = False):
    """key_switch_batch: (chunks, whether the level sum was formed in k_k3)"""
    c = min(chunk, n or 1)
    if sum_out:
        if c < group_size or not fuse_pays(ch, group_size, L):
            sum_out = False
        else:
            c -= c % group_size
    dual = may_dual and n > c
    chunks, off, ci = [], 0, 0
    while off < n:
        nc = min(c, n - off)
        cp = plan_chunk(ch, L, nc, kind, out_apart, rescale, group_size, sum_out, coeff)
        cp.off, cp.stream = off, (ci & 1) if dual else 0
        chunks.append(cp)
        off += c
        ci += 1
    return chunks, sum_out


# ---- rotations: NAF terms, the trie of rotate_sum, the term groups of rotate_each -------------------------------------------------------
def naf_terms(step: int, N: int) -> list:
    """Evaluator::rotate_internal's terms, least significant first; a term of N / 2 is no rotation"""
    neg, v, i, out = step < 0, abs(step), 0, []
    while v:
        z = 2 - (v & 3) if v & 1 else 0
        v = (v - z) >> 1
        if z and (1 << i) != N // 2:
            out.append((-z if neg else z) * (1 << i))
        i += 1
    return out


def rotation_terms(step: int, N: int, key_steps) -> list:
    """a step with a Galois key of its own is one term (key_steps: the steps whose elements have keys)"""
    if step == 0:
        return []
    return [step] if step in key_steps else naf_terms(step, N)


def rotation_trie_levels(steps, N: int, key_steps) -> list:
    """[number of nodes of trie level 1, 2, ...] (rotation_trie; two steps share the prefix of their term sequences)"""
    seen, widths = set(), {}
    for s in steps:
        terms = tuple(rotation_terms(s, N, key_steps))
        for d in range(1, len(terms) + 1):
            if terms[:d] not in seen:
                seen.add(terms[:d])
                widths[d] = widths.get(d, 0) + 1
    return [widths[d] for d in sorted(widths)]


def rotation_trie_nodes(steps, N: int, key_steps) -> dict:
    """{term prefix: [steps ending there, has children]}"""
    nodes = {}
    for s in steps:
        terms = tuple(rotation_terms(s, N, key_steps))
        for d in range(1, len(terms) + 1):
            e = nodes.setdefault(terms[:d], [0, False])
            if d < len(terms):
                e[1] = True
        if terms:
            nodes[terms][0] += 1
    return nodes


# ---- one call of the C API --------------------------------------------------------------------------------------------------------------
OPS = {
    # name: (key-switch kind, rescale, out_apart)
    "multiply_relin": ("product", False, True),
    "multiply_relin_over_a": ("product", False, False),
    "multiply_relin_rescale": ("product", True, True),
    "multiply_relin_rescale_over_a": ("product", True, False),
    "relinearize": ("size3", False, True),
    "relinearize_rescale": ("size3", True, True),
    "apply_galois": ("galois", False, True),
    "rotate_add_in_place": ("galois", False, True),  # (a rotation may add into `out`: always apart)
    "rotate_sum": ("grouped", False, True),
    "rotate_each": ("grouped", False, True),
}
ROTATE_KEY_STEPS = (1, 2, 4, -1)   # the steps whose Galois keys the rotation cases install
ROTATE_SUM_STEPS = (1, 2, 3)       # 3 = -1 + 4: a NAF term under a one-term node, a trie of two levels
EACH_STEPS = (1, 2, 3, 5)          # rotate_each: row r rotates by EACH_STEPS[r % 4] (5 = 1 + 4)


def plan_call(ch: Chain, op: str, L: int, n: int, chunk: int = DEFAULT_CHUNK, dual_stream: bool = True, level_walk: bool = True,
              steps=None, key_steps=ROTATE_KEY_STEPS) -> CallPlan:
    kind, rescale, apart = OPS[op]
    bfv = ch.scheme == "bfv"
    cp = CallPlan(op, L, n, apart)
    if op == "rotate_sum":
        _plan_rotate_sum(cp, ch, L, n, chunk, level_walk, tuple(steps or ROTATE_SUM_STEPS), key_steps)
    elif op == "rotate_each":
        _plan_rotate_each(cp, ch, L, n, chunk, level_walk, [EACH_STEPS[r % len(EACH_STEPS)] for r in range(n)] if steps is None else list(steps), key_steps)
    else:
        may_dual = dual_stream and kind == "product"
        cp.chunks, _ = plan_batch(ch, L, n, kind, apart, rescale, chunk, may_dual, coeff=bfv)
    return cp


def _plan_rotate_sum(cp, ch, L, n, chunk, level_walk, steps, key_steps):
    bfv = ch.scheme == "bfv"
    widths = rotation_trie_levels(steps, ch.N, key_steps)
    nodes = rotation_trie_nodes(steps, ch.N, key_steps)
    cp.key_switches = len(nodes)
    if not nodes:
        return
    widest = max(widths + [1])
    if not level_walk or not k3_can_fuse(ch) or latency_shape(ch, n * widest, ntt_pipeline=not bfv):
        for _ in nodes:  # node by node: one apply_galois each (a BFV context: the coefficient-form key switch)
            chunks, _ = plan_batch(ch, L, n, "galois", True, False, chunk, False, coeff=bfv)
            cp.chunks += chunks
        return
    for G in widths:
        in_k3 = level_sum_pays(ch, L, n, chunk)
        chunks, summed = plan_batch(ch, L, G * n, "grouped", True, False, chunk, False, group_size=n, sum_out=in_k3)
        cp.chunks += chunks
        if summed:
            cp.level_sums_in_k3 += 1
        else:
            cp.level_sums_by_kernel += 1


def _plan_rotate_each(cp, ch, L, n, chunk, level_walk, steps, key_steps):
    bfv = ch.scheme == "bfv"
    terms = [rotation_terms(s, ch.N, key_steps) for s in steps]
    for t in range(max((len(x) for x in terms), default=0)):
        groups = {}
        for x in terms:
            if t < len(x):
                groups[x[t]] = groups.get(x[t], 0) + 1
        m_all = sum(groups.values())
        if not bfv and level_walk and k3_can_fuse(ch) and not latency_shape(ch, m_all) and len(groups) > 1:
            chunks, _ = plan_batch(ch, L, m_all, "grouped", True, False, chunk, False, group_size=1)
            cp.chunks += chunks
        else:
            for e in sorted(groups, key=lambda s: galois_elt(s, ch.N)):  # (std::map over the Galois elements)
                chunks, _ = plan_batch(ch, L, groups[e], "galois", True, False, chunk, False, coeff=bfv)
                cp.chunks += chunks


def galois_elt(step: int, N: int) -> int:
    """GaloisTool::get_elt_from_step: 3^step mod 2N for a left rotation by step (a negative step: by N / 2 - |step|); 0: the conjugation"""
    m = 2 * N
    if step == 0:
        return m - 1
    pos = step if step > 0 else (N >> 1) - (-step)
    return pow(3, pos, m)


# ---- decisions --------------------------------------------------------------------------------------------------------------------------
DECISIONS = {
    "shape": ("lds", "latency", "unfused", "fused"),
    "out_apart": ("yes", "no"),
    "k_k1": ("dual", "per_engine"),
    "k_k2n": ("dual", "per_digit_kind"),
    "ts": (1, 2, 4),
    "og_per_block": (1, 2, 4),
    "u64_waves": (4, 8),
    "k_k3": ("dual8", "separate"),
    "floor_rows": ("dual", "per_engine"),
    "level_sum": ("in_k3", "by_kernel"),
    "og_tail": (1, 2, 3, 4, 5, 6, 7),
}


def outcomes(ch: Chain, plan: CallPlan) -> set:
    """{(decision, outcome)} one call's plan takes.  Launch-level decisions count where the rule had a choice: both engines (digit kinds)
    present for the dual rules, the throughput shapes for ts / og_per_block / waves / op-group tails."""
    out = {("out_apart", "yes" if plan.out_apart else "no")}
    for c in plan.chunks:
        if c.shape == "bfv_coeff":
            continue
        out.add(("shape", c.shape))
        if c.shape not in ("fused", "unfused"):
            continue
        if c.nc % 8:
            out.add(("og_tail", c.nc % 8))
        both = any(ch.fp64[:plan.L]) and not all(ch.fp64[:plan.L])
        kinds = len({b >= 53 for b in ch.bits[:plan.L]}) == 2
        k3_calls = {}
        for l in c.launches:
            if l.family in ("k_k1", "k_k1_dual") and both:
                out.add(("k_k1", "dual" if l.family.endswith("dual") else "per_engine"))
            elif l.family in ("k_k2n", "k_k2n_dual"):
                out.add(("ts", l.ts))
                if kinds:
                    out.add(("k_k2n", "dual" if l.family.endswith("dual") else "per_digit_kind"))
            elif l.family in ("k_floor_rows", "k_floor_rows_dual") and not l.note:  # (with a tail prime the rule has no choice)
                if l.family.endswith("dual"):
                    out.add(("floor_rows", "dual"))
                elif l.engine == "u64" and both:
                    out.add(("floor_rows", "per_engine"))
            elif l.family == "k_k3_dual8":
                out.add(("k_k3", "dual8"))
                out.add(("u64_waves", l.waves))
                if not c.level_sum or "special" in l.note:
                    for w in l.note.split("og_per_block")[1].split()[1::2]:
                        out.add(("og_per_block", int(w)))
            elif l.family == "k_k3":
                k3_calls.setdefault(l.note, []).append(l)
                if l.engine == "u64":
                    out.add(("u64_waves", l.waves))
                if not c.level_sum or "special" in l.note:
                    out.add(("og_per_block", l.og_per_block))
        if any(len(v) == 2 for v in k3_calls.values()):
            out.add(("k_k3", "separate"))
    if plan.level_sums_in_k3:
        out.add(("level_sum", "in_k3"))
    if plan.level_sums_by_kernel:
        out.add(("level_sum", "by_kernel"))
    return out


def boundary_cases(ch: Chain, op: str, L: int | None = None, decisions=None, scan_max: int = SCAN_MAX, chunk: int = DEFAULT_CHUNK) -> list:
    """The batch sizes that pin op's selection rules on this chain: for every decision the chain reaches with n <= scan_max (`decisions`:
    only those named -- a large ring is held to what no smaller one reaches), and every outcome of it, the smallest n that takes the
    outcome and the n just below it, which does not; and where a throughput shape is first taken, the first multiple of 8 above the
    last batch of the other side with its two neighbours: 8k - 1, 8k, 8k + 1.  Sorted, without duplicates."""
    L = ch.Ltop if L is None else L
    first, ns = set(), set()
    for n in range(1, scan_max + 1):
        for o in sorted(outcomes(ch, plan_call(ch, op, L, n, chunk)), key=str):
            if o[0] == "og_tail" or o in first or (decisions is not None and o[0] not in decisions):
                continue
            first.add(o)
            ns.add(n)
            if n > 1:
                ns.add(n - 1)
                if o[0] == "shape" and o[1] in ("unfused", "fused"):
                    k8 = (n - 1) // 8 * 8 + 8  # the first multiple of 8 above the last batch of the lower side
                    ns.update(x for x in (k8 - 1, k8, k8 + 1) if x <= scan_max)
    return sorted(ns)


def describe(ch: Chain, plan: CallPlan) -> str:
    parts = []
    for c in plan.chunks:
        ls = " ".join(f"{l.family}[{l.grid[0]}" + (f"x{l.grid[1]}" if l.grid[1] > 1 else "") + "]" for l in c.launches)
        parts.append(f"{c.shape}({c.nc}): {ls}")
    return "; ".join(parts)


# ---- the case table of tests/test_gpu_selection_boundaries.py ----------------------------------------------------------------------------
HEADLINE_BITS = (60,) + (45,) * 15 + (60,)
CHAINS = {
    # name: (scheme, N, key-level bit sizes) -- the smallest chains that reach the decisions
    "n8192_60_45_60_both_engines": ("ckks", 8192, (60, 45, 60)),              # LDS / unfused / fused, every dual rule
    "n4096_60_60_60_u64_engine": ("ckks", 4096, (60, 60, 60)),                # no dual launches: the u64 engine's own grids
    "n4096_46_45_46_fp64_engine": ("ckks", 4096, (46, 45, 46)),               # no dual launches: the fp64 engine's own grids
    "n16384_60_45_45_45_60_L4": ("ckks", 16384, (60, 45, 45, 45, 60)),        # no LDS shape: latency / unfused / fused
    "n32768_headline": ("ckks", 32768, HEADLINE_BITS),                        # L = 16 and L = 15: where fuse_pays' second clause decides
    "bfv_n8192_60_40_60": ("bfv", 8192, (60, 40, 60)),                        # the grouped NTT-domain path of a BFV context
    # the Shoup build of the u64 engine (tests/shoup_rings.py holds the chains): the same rules, other machine code
    "n16384_60_50_40_60_shoup": ("ckks", 16384, (60, 50, 40, 60)),            # LOGN1 = 4: latency / unfused / fused, every dual rule
    "n8192_60_50_40_60_shoup": ("ckks", 8192, (60, 50, 40, 60)),              # LOGN1 = 3: the ring-in-LDS shape as well
    "n16384_60_50_60_shoup": ("ckks", 16384, (60, 50, 60)),                   # no fp64 prime: no dual launches
}
SHOUP_CHAINS = tuple(k for k in CHAINS if k.endswith("_shoup"))  # each is an entry of shoup_rings.RINGS under the same name
ALL_BUT_OG = tuple(d for d in DECISIONS if d != "og_per_block")
CASES = [
    # (chain, op, L or None for the top level, decisions to pin or None for every one the chain reaches)
    ("n8192_60_45_60_both_engines", "multiply_relin", None, None),
    ("n8192_60_45_60_both_engines", "multiply_relin_over_a", None, None),
    ("n8192_60_45_60_both_engines", "multiply_relin_rescale", None, None),
    ("n8192_60_45_60_both_engines", "multiply_relin_rescale_over_a", None, None),
    ("n8192_60_45_60_both_engines", "relinearize", None, None),
    ("n8192_60_45_60_both_engines", "relinearize_rescale", None, None),
    ("n8192_60_45_60_both_engines", "apply_galois", None, None),
    ("n8192_60_45_60_both_engines", "rotate_add_in_place", None, None),
    ("n8192_60_45_60_both_engines", "rotate_sum", None, None),
    ("n8192_60_45_60_both_engines", "rotate_each", None, None),
    ("n4096_60_60_60_u64_engine", "multiply_relin_rescale", None, None),
    ("n4096_60_60_60_u64_engine", "multiply_relin_over_a", None, None),
    ("n4096_60_60_60_u64_engine", "relinearize_rescale", None, None),
    ("n4096_60_60_60_u64_engine", "rotate_sum", None, ALL_BUT_OG),
    ("n4096_46_45_46_fp64_engine", "multiply_relin_rescale", None, None),
    ("n4096_46_45_46_fp64_engine", "multiply_relin_over_a", None, None),
    ("n4096_46_45_46_fp64_engine", "apply_galois", None, None),
    ("n4096_46_45_46_fp64_engine", "rotate_each", None, None),
    ("n16384_60_45_45_45_60_L4", "multiply_relin_rescale", None, None),
    ("n16384_60_45_45_45_60_L4", "multiply_relin_rescale_over_a", None, None),
    ("n16384_60_45_45_45_60_L4", "relinearize", None, None),
    ("n16384_60_45_45_45_60_L4", "rotate_sum", None, ALL_BUT_OG),  # (k_k3's separate launches: 3 x 171 ciphertexts in one grouped launch)
    ("n16384_60_45_45_45_60_L4", "rotate_each", None, None),
    ("n32768_headline", "multiply_relin_rescale", 16, ("shape",)),
    ("n32768_headline", "rotate_add_in_place", 16, ("shape",)),
    ("n32768_headline", "multiply_relin", 15, ("shape",)),
    ("n32768_headline", "apply_galois", 15, ("shape",)),
    ("n16384_60_50_40_60_shoup", "multiply_relin_rescale", None, None),
    ("n16384_60_50_40_60_shoup", "multiply_relin_rescale_over_a", None, None),
    ("n16384_60_50_40_60_shoup", "relinearize", None, None),
    ("n16384_60_50_40_60_shoup", "apply_galois", None, None),
    ("n16384_60_50_40_60_shoup", "rotate_sum", None, ALL_BUT_OG),
    ("n16384_60_50_40_60_shoup", "rotate_each", None, None),
    ("n8192_60_50_40_60_shoup", "multiply_relin_rescale", None, None),
    ("n8192_60_50_40_60_shoup", "relinearize_rescale", None, None),
    ("n8192_60_50_40_60_shoup", "rotate_add_in_place", None, None),
    ("n8192_60_50_40_60_shoup", "rotate_sum", None, ALL_BUT_OG),
    ("n16384_60_50_60_shoup", "multiply_relin_rescale", None, None),
    ("n16384_60_50_60_shoup", "rotate_sum", None, ALL_BUT_OG),
    # (the BFV chain last, its coefficient-form key switch -- no counter, no planned launches -- the last row of all: tools/plan_vs_trace.py
    # deals the traced dispatches to the calls in order, and what that row dispatches is planned by nobody)
    ("bfv_n8192_60_40_60", "rotate_sum", None, None),
    ("bfv_n8192_60_40_60", "relinearize", None, None),
]


def case_chain(name: str, fp64=None) -> Chain:
    scheme, N, bits = CHAINS[name]
    return chain(scheme, N, bits, fp64)


def case_level(name: str, L) -> int:
    return case_chain(name).Ltop if L is None else L


def case_table(fp64_of=None) -> list:
    """[(chain name, op, L, [batch sizes])] -- fp64_of: {chain name: engines of a device context} (else the restated engine rule)"""
    rows = []
    for name, op, L, dec in CASES:
        ch = case_chain(name, (fp64_of or {}).get(name))
        rows.append((name, op, case_level(name, L), boundary_cases(ch, op, case_level(name, L), dec)))
    return rows


def mixed_shape_calls(ch: Chain, L: int) -> list:
    """[(op, chunk, n)]: calls whose body chunks take a throughput shape and whose ragged last chunk takes the LDS shape (`out` apart) or
    the latency shape (`out` over operand a).  The chunk is the first multiple of 8 that takes the throughput shape in either layout, once
    for the unfused and once for the fused shape; the tail is the largest odd batch that both small shapes still hold, at most 5; two body
    chunks, so that with two streams they alternate."""
    tail = min(5, lds_limit(ch, L), lat_limit(ch))
    tail -= 1 - tail % 2
    out = []
    for shape in ("unfused", "fused"):
        c = next(8 * k for k in range(1, 129) if all(ks_shape(ch, L, 8 * k, "product", apart) == shape for apart in (True, False)))
        for op in ("multiply_relin_rescale", "multiply_relin_rescale_over_a"):
            out.append((op, c, 2 * c + tail))
    return out
