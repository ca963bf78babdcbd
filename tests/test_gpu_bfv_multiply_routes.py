"""he355_bfv_multiply (BEHZ) on every route its host-side kernel selection can take and on every instantiation of its fused column kernels,
bit-exact (np.array_equal, no tolerance) against oracle.bfv_multiply -- itself held to the exact integer model at these kinds of level and
operand in test_oracle_bfv_multiply_model_cpu.py.  tests/bfv_multiply_plan.py restates the selection (its CPU test pins it to the numbers
of the launchers and shows that the case table below takes every outcome of every decision and all nine instantiations); every call here
resets he355_bfv_multiply_stats first and asserts afterwards that the counters equal the plan's, so a result cannot pass on another route
than the one meant.  Printed per call: `routes <chain> L = <level> <case>: ...`.

Chains and levels (bfv_multiply_plan.CHAINS): N = 2048 / 4096 (<1,..> / <2,..>, the latter also at nB = 1), N = 8192 at {60,40,40,40}
L = 4 / 3 / 2 (the three EXACT instantiations) and L = 1 (<3,4,6,false>), at five data primes (L = 5: the unfused <16,24> kernels at a
fusable ring size; L = 4 fused, same context), at {60 x 4} (every data prime on the u64 engine), in the Shoup form ({50,40}), under
HE355_FORCE_U64=1 and HE355_BEHZ_BASE=seal (one engine for every or nearly every residue; the integer Shenoy-Kumaresan form);
N = 16384 (<4,..>: 1024-thread blocks) at 32 / 40 / 56 KiB, exactly 64 KiB, 72 KiB and 88 KiB of dynamic LDS -- above 64 KiB the launchers
ask the runtime for the opt-in, and where a device does not grant it the plan (fed the device's own `lds_limit`) expects the unfused route;
N = 32768 and N = 1024 (unfused <4,6>) at the top level and at L = 1.

Operands, for every chain and level: the seven family ciphertexts of bfv_multiply_operands.py built for the level's own Q (all
+floor(Q/2), all -floor(Q/2), alternating, first-negative, Q - 1, 0 and 1) and two uniform ones; every call shape mixes them.
Call shapes (bfv_multiply_plan.boundary_cases): an outer product 3 x 2 (lists path), a ragged outer product n = 5, b1 = 2, pairwise n = 3
(per-pair path), n = 1, an outer product 2 x 3 in chunks of 4 (the first chunk ends inside a row, the last is ragged), pairwise n = 3 in
chunks of 2.  On n8192_default at L = 2, n16384_d3 at L = 3 and n8192_shoup at L = 1 additionally the batches on both sides of the two
1024-block rules (per-pair 25 | 26, 9 | 10 and 42 | 43 results, lists 34 | 35, 12 | 13 and 56 | 57; the last chain's split sides are 1032 and
1026 blocks, the closest any chain here comes to the constant from above), each once after a smaller and once after a larger call in the
same context, so that a scratch layout left by another batch size shows.  Every product of every call is checked against the oracle (no
threshold batch has more than 57 results: no share is sampled).

Every output lies between a ring's worth of sentinel words before and after it; every operand is read back.
Not run: LOGN1 = 4 in the Shoup form, and the halving of a chunk when the arena does not fit."""
import os

import numpy as np
import pytest

import bfv_multiply_plan as mp
import shoup_rings as sr
from bfv_gpu_helpers import SENT, At, be  # noqa: F401 (be: the fixture)
from bfv_multiply_operands import family_cts

pytestmark = pytest.mark.gpu

LEVELS = [(name, L) for name, spec in mp.CHAINS.items() for L in spec[3]]
THRESHOLD_LEVELS = [(name, L) for name, spec in mp.CHAINS.items() for L in spec[4]]


@pytest.fixture(scope="module")
def contexts(be, oracle):
    """{chain: (g, o)} made on first use, the environment set around context creation (test_gpu_edge_operands.make_pair); closed with the module"""
    made = {}

    def get(name):
        if name not in made:
            (N, bits, pb), force, seal, _, _ = mp.CHAINS[name]
            env = {"HE355_FORCE_U64": "1" if force else None, "HE355_BEHZ_BASE": "seal" if seal else None}
            saved = {k: os.environ.get(k) for k in env}
            try:
                for k, v in env.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
                g = be.Context(be.SCHEME_BFV, N, bit_sizes=list(bits), plain_bits=pb, sec128=False, device=0)
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            o = oracle.Context(oracle.SCHEME_BFV, N, bit_sizes=list(bits), plain_bits=pb, sec128=False)
            assert g.moduli == o.moduli and g.t == o.t
            if force:
                assert not any(g.fp64)
            if name in mp.SHOUP_RINGS:  # the Shoup build of the u64 engine: the chain's form, engines and plain modulus are the table's
                sr.check_device(mp.SHOUP_RINGS[name], g)
                sr.check(mp.SHOUP_RINGS[name], o.moduli, g.t)
            made[name] = (g, o)
        return made[name]

    yield get
    for g, _ in made.values():
        g.close()


class Level:
    """one (chain, level): the operand pool, the oracle's products of it (each computed once) and the calls"""

    def __init__(self, get, name, L):
        self.g, self.o = get(name)
        self.name, self.L, self.N = name, L, self.g.N
        self.lv = mp.chain_levels(name)[L]
        assert self.lv.N == self.N and 1 <= L <= self.g.L
        rng = np.random.default_rng(7000 + 10 * self.N + L)
        self.pool = family_cts(self.o, L, self.N) + [self.o.random_poly(rng, L, 2) for _ in range(2)]
        self.memo = {}
        self.lds_limit = self.g.bfv_multiply_stats()["lds_limit"]
        assert self.lds_limit >= mp.LDS_NO_OPT_IN

    def want(self, ia, ib):
        if (ia, ib) not in self.memo:
            self.memo[ia, ib] = self.o.bfv_multiply(self.pool[ia], self.pool[ib])
        return self.memo[ia, ib]

    def operands(self, case):
        """(pool indices of the a slab, of the b slab, [(a slab index, b slab index) of result r])"""
        P = len(self.pool)
        fixed = {"outer_3x2": ([0, 1, 2], [3, 4]), "outer_ragged_5": ([0, 1, 2], [3, 4]), "outer_2x3_chunk4": ([5, 6], [6, 7, 8]),
                 "pairwise_3": ([4, 0, 8], [4, 1, 7]), "pairwise_3_chunk2": ([4, 0, 8], [4, 1, 7]), "single": ([2], [2])}
        if case.kind == "pairwise":
            a, b = fixed.get(case.name) or ([r % P for r in range(case.n)], [(2 * r + 1 + r // P) % P for r in range(case.n)])
            return a, b, [(r, r) for r in range(case.n)]
        rows = -(-case.n // case.b1)
        a, b = fixed.get(case.name) or ([(i + 7) % P for i in range(rows)], [(3 * j + 2) % P for j in range(case.b1)])
        assert len(a) == rows and len(b) == min(case.b1, case.n)
        return a, b, [(r // case.b1, r % case.b1) for r in range(case.n)]

    def run(self, be, case, note=""):
        g, L, N = self.g, self.L, self.N
        a_idx, b_idx, of = self.operands(case)
        a, b = np.stack([self.pool[i] for i in a_idx]), np.stack([self.pool[i] for i in b_idx])
        da, db = g.to_device(a), g.to_device(b)
        buf = g.to_device(np.full(case.n * 3 * L * N + 2 * N, SENT, dtype=np.uint64))
        ix = be.Context.pairwise() if case.kind == "pairwise" else be.Context.outer(0, len(a_idx), 0, case.b1)
        what = (self.name, L, case.name, note)
        g.set_chunk(case.chunk)
        try:
            g.bfv_multiply_stats(reset=True)
            g.bfv_multiply(L, case.n, da, db, ix, At(buf, N))
            stats = g.bfv_multiply_stats()
        finally:
            g.set_chunk(mp.DEFAULT_CHUNK)
        got = buf.download()
        assert stats.pop("lds_limit") == self.lds_limit
        print(f"routes {self.name} L = {L} {case.name}{note}: " + ", ".join(f"{k} = {c}" for k, c in stats.items() if c)
              + f"; columns {mp.instantiation(self.lv, self.lds_limit)}, {self.lv.lds_bytes / 1024:g} of {self.lds_limit // 1024} KiB of LDS")
        # the route first: a result on another route than the plan's is not the one this case means to check
        assert stats == mp.plan(self.lv, case.n, *mp.indexer(case.kind, case.b1), case.chunk, self.lds_limit), (what, "counters", stats)
        assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), (what, "sentinel")
        got = got[N:-N].reshape(case.n, 3, L, N)
        for r, (ra, rb) in enumerate(of):
            ref = self.want(a_idx[ra], b_idx[rb])
            assert np.array_equal(got[r], ref), (what, "result", r, np.argwhere(got[r] != ref)[:1].tolist())
        assert np.array_equal(da.download(a.shape), a) and np.array_equal(db.download(b.shape), b), (what, "operands")
        for x in (da, db, buf):
            x.free()


@pytest.mark.parametrize("name,L", LEVELS, ids=[f"{n}-L{L}" for n, L in LEVELS])
def test_every_call_shape_on_the_level_s_route(be, contexts, name, L):
    lvl = Level(contexts, name, L)
    for case in mp.boundary_cases(lvl.lv):
        lvl.run(be, case)


@pytest.mark.parametrize("name,L", THRESHOLD_LEVELS, ids=[f"{n}-L{L}" for n, L in THRESHOLD_LEVELS])
def test_both_sides_of_the_1024_block_rules(be, contexts, name, L):
    """the per-pair path on either side of k_behz_rows_tensor_dual's rule and the lists path on either side of k_behz_tensor_inv_dual's, each
    after a smaller call (n = 1) and after a larger one (pairwise, three results more than the largest batch) in the same context"""
    lvl = Level(contexts, name, L)
    cases = mp.boundary_cases(lvl.lv, with_thresholds=True)
    small = next(c for c in cases if c.name == "single")
    batches = [c for c in cases if c.name.startswith(("rows_", "inv_"))]
    assert [c.name.rsplit("_", 1)[0] for c in batches] == ["rows_dual", "rows_split", "inv_dual", "inv_split"]
    assert max(c.n for c in batches) <= 60  # every product of every batch is checked against the oracle
    large = mp.Case("larger", "pairwise", max(c.n for c in batches) + 3, 1, mp.DEFAULT_CHUNK)
    for case in batches:
        lvl.run(be, small, " (before)")
        lvl.run(be, case, " after n = 1")
        lvl.run(be, large, " (before)")
        lvl.run(be, case, f" after n = {large.n}")


def test_multiply_relin_accumulate_counts_through_the_same_code(be, oracle, contexts):
    """he355_bfv_multiply_relin_accumulate(rows 2, cols 2, inner 2): one multiply of 8 results in groups of 4 with rows of 2 -- the lists path --
    counted by he355_bfv_multiply_stats as he355_bfv_multiply's calls are; the sums against the oracle's loop"""
    name, rows, cols, inner = "n4096_d3", 2, 2, 2
    g, o = contexts(name)
    L, N = g.L, g.N
    lv = mp.chain_levels(name)[L]
    rng = np.random.default_rng(7100)
    rk = o.random_kswitch_key(rng)
    g.set_relin_key(rk)
    A = np.stack([o.random_poly(rng, L, 2) for _ in range(rows * inner)])  # a(i, k) at k rows + i
    B = np.stack([o.random_poly(rng, L, 2) for _ in range(inner * cols)])  # b(k, j) at k cols + j
    dA, dB = g.to_device(A), g.to_device(B)
    buf = g.to_device(np.full(rows * cols * 2 * L * N + 2 * N, SENT, dtype=np.uint64))
    g.bfv_multiply_stats(reset=True)
    g.bfv_multiply_relin_accumulate(L, rows, cols, inner, dA, 1, rows, dB, cols, 1, At(buf, N))
    stats = g.bfv_multiply_stats()
    lds_limit = stats.pop("lds_limit")
    print(f"routes {name} L = {L} relin_accumulate 2 x 2 x 2: " + ", ".join(f"{k} = {c}" for k, c in stats.items() if c))
    assert stats == mp.plan(lv, rows * cols * inner, rows * cols, cols, mp.DEFAULT_CHUNK, lds_limit) and stats["calls_lists"] == 1
    got = buf.download()
    assert (got[:N] == SENT).all() and (got[-N:] == SENT).all(), "sentinel"
    got = got[N:-N].reshape(rows * cols, 2, L, N)
    for i in range(rows):
        for j in range(cols):
            want = None
            for k in range(inner):
                term = o.relinearize(o.bfv_multiply(A[k * rows + i], B[k * cols + j]), rk)
                want = term if want is None else o.add(want, term)
            assert np.array_equal(got[i * cols + j], want), (i, j)
    assert np.array_equal(dA.download(A.shape), A) and np.array_equal(dB.download(B.shape), B), "operands"
    for x in (dA, dB, buf):
        x.free()
