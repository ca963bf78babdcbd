"""The kernels held to the oracle, bit for bit (np.array_equal), on moduli the prime-size rule never makes: the chains of
tests/golden/explicit_moduli.json (tests/explicit_moduli.py says what each is for; tests/test_explicit_moduli_cpu.py holds the fixture's
properties and the oracle itself on them).  Run with -m gpu on an MI355X; nothing here skips.

CKKS, every chain with t = 0:
  * multiply, multiply_plain, multiply_accumulate over 33 `qm1` terms, rescale (sizes 2 and 3), mod_switch_drop, ntt_forward / ntt_inverse;
  * the key switches -- multiply_relin with and without rescale, relinearize, relinearize_rescale, rotate, rotate_add, rotate_sum -- under
    every shape the chain has: ring-in-LDS and latency (N <= 8192 and L <= 6: a batch of 5 in ragged chunks of 2, the latency shape with
    the LDS shape switched off; elsewhere the batch the library's own rule gives the latency shape), and the fused throughput shape at
    the smallest ragged batch tests/launch_plan.py calls "fused", rows tiled from 7 distinct ones.  he355_path_stats must equal the plan;
  * keys: uniform for every op; all-(q - 1), identity on the first digit and identity on the last digit for relinearize,
    multiply_relin_rescale and rotate at the top level -- the identity keys against the closed form in Python integers
    (edge_operands.identity_key_switch) as well; on xbound_* the all-(q - 1) keys one level below the top too (terms == acc_terms);
  * operands: `qm1`, `qm1_coeff`, `planted` and uniform rows; on fits48_inside_* one row carries the hill-climbed worst column of the
    inside digit under the inside target (edge_operands.worst_column / column_digit).  It reaches the digit lift as an intact column
    under relinearize and relinearize_rescale (it is c2 of the size-3 operand); a rotation permutes it first, so there it is one more
    structured operand, not the searched worst case;
  * xbound_*: one level below the top (the c1 sums of a ct x ct launch hold exactly acc_terms terms) and at the top (one more), and
    rotate_sum with the level sums inside k_k3 (asserted).

BFV, the twins (every t of the fixture: 2, 256, 2^31, 2^32 - 5, the largest batching prime, 3 * 12289): encrypt, decrypt, bfv_multiply,
relinearize, bfv_multiply_relin_accumulate (the fused multiply -> relinearize -> add, 2 results of 3 terms), bfv_mod_switch,
bfv_add_plain / sub_plain, bfv_multiply_plain, bfv_multiply_plain_accumulate over more terms than the shortest run, bfv_noise_budget; plaintext coefficients 0, 1, floor(t/2), floor(t/2) + 1, t - 1; phases on both sides of the tie points
of the rounding (client_operands.planted_phases).  he355_bfv_encode / he355_bfv_decode are refused under a non-batching t and work
under the batching one.

Every call prints its counters (`paths <chain> ...`); profiles/explicit_moduli.txt holds one run's output."""
import importlib
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bfv_noise_model as noise  # noqa: E402
import client_operands as co  # noqa: E402
import edge_operands as eo  # noqa: E402
import explicit_moduli as xm  # noqa: E402
import launch_plan as lp  # noqa: E402
import sampler_np as sn  # noqa: E402
from bfv_gpu_helpers import At, inner_of, lift, pair, refused, sentinelled  # noqa: E402
from bfv_multiply_operands import family_cts  # noqa: E402

_SHAPE_ENV = ("HE355_CHUNK", "HE355_LATENCY_MAX", "HE355_LEVEL_WALK", "HE355_LDS_MAX", "HE355_FORCE_U64")
DEFAULT_SHAPES = not any(os.environ.get(k) for k in _SHAPE_ENV)
CH = xm.load()
CKKS = [k for k, c in CH.items() if not c["t"] and c["N"] > 1024]
BFV = [k for k, c in CH.items() if c["t"] and c["N"] > 1024]
FAM = ["qm1", None, "qm1_coeff", "planted", None, None, None]  # the first five: the small batch; row r of a tiled batch holds r mod 7
WORST_ROW = 4
KS_OPS = ["multiply_relin", "multiply_relin_rescale", "relinearize", "relinearize_rescale", "rotate", "rotate_add", "rotate_sum"]
PLAN_OP = {"rotate": "apply_galois", "rotate_add": "rotate_add_in_place"}
KEY_KINDS = ["qm1", "identity_first", "identity_last"]
KEY_OPS = ["relinearize", "multiply_relin_rescale", "rotate"]
T0 = time.time()


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need an MI355X (the backend has no CPU fallback)")
    return mod


def levels(cid):
    Ltop = len(CH[cid]["primes"]) - 1
    return [Ltop - 1, Ltop] if cid.startswith("xbound") else [Ltop]


def shapes(cid, L):
    return (["lds"] if CH[cid]["N"] <= 8192 and L <= 6 else []) + ["latency", "fused"]


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} words differ from the oracle, first at {at}: got {int(got[at])}, want {int(want[at])}")


class State:
    """one chain's device and oracle contexts, its keys by kind, 7 distinct operand rows per level and the oracle's results"""

    def __init__(self, be, ho, cid):
        c = CH[cid]
        self.be, self.ho, self.cid, self.N = be, ho, cid, c["N"]
        self.primes = c["primes"]
        self.g = be.Context(be.SCHEME_CKKS, self.N, primes=self.primes, device=0)
        self.o = o = ho.Context(ho.SCHEME_CKKS, self.N, primes=self.primes)
        assert self.g.moduli == o.moduli == self.primes, (cid, "the library admits every chain of the fixture")
        assert self.g.fp64 == [xm.is_f64(q) for q in self.primes]
        self.chain = lp.chain("ckks", self.N, xm.bits_of(self.primes), self.g.fp64)
        self.rng = np.random.default_rng(sum(self.primes) % (2 ** 32))
        self.steps = lp.ROTATE_KEY_STEPS
        self.keys, self.kind = {}, None
        self.host, self.dev, self.want = {}, {}, {}
        self.worst = None
        if cid.startswith("fits48_inside"):
            self.worst = eo.worst_column(self.N, None, c["digit"], c["target"], uniform_columns=1000, primes=self.primes, restarts=2)
            print(f"paths {cid} worst column of digit {c['digit']} under target {c['target']}: 2^{np.log2(self.worst['magnitude']):.4f} "
                  f"of a bound of 2^{np.log2(self.worst['bound']):.4f}")
        self.use("uniform")

    def close(self):
        self.g.close()

    def j0(self, kind):
        return {"identity_first": 0, "identity_last": self.o.L - 1}[kind]

    def use(self, kind):
        """the relinearization key and the Galois keys of `kind`, on the device"""
        if kind not in self.keys:
            o = self.o
            if kind.startswith("identity"):
                k = eo.key(o, "identity", j0=self.j0(kind))
                self.keys[kind] = (k, {o.galois_elt(s): k for s in self.steps})
            else:
                self.keys[kind] = (eo.key(o, kind, self.rng), {o.galois_elt(s): eo.key(o, kind, self.rng) for s in self.steps})
        if self.kind != kind:
            rk, gks = self.keys[kind]
            self.g.set_relin_key(rk)
            for e, k in gks.items():
                self.g.set_galois_key(e, k)
            self.kind = kind
        return self.keys[kind]

    def operands(self, L):
        if L not in self.host:
            o = self.o
            A = eo.batch(o, FAM, L, 2, self.rng)
            B = eo.batch(o, FAM[::-1], L, 2, self.rng)
            C3 = np.stack([o.multiply_ntt(A[i], B[i]) for i in range(len(FAM))])
            if self.worst is not None:  # c2 of the size-3 operand: the relinearization's digits are this column (a rotation permutes its c1 first)
                poly = eo.column_digit(o, L, CH[self.cid]["digit"], self.worst["column"])
                A[WORST_ROW] = np.stack([poly, poly])
                C3[WORST_ROW] = o.multiply_ntt(A[WORST_ROW], B[WORST_ROW])
                C3[WORST_ROW, 2] = poly
            self.host[L] = (A, B, C3)
        return self.host[L]

    def slabs(self, L, n):
        """the rows r mod 7 of A, B, C3 on the device, once per (L, n)"""
        if (L, n) not in self.dev:
            for k in [k for k in self.dev if k[1] > 8]:  # one large batch at a time
                for b in self.dev.pop(k):
                    b.free()
            idx = np.arange(n) % len(FAM)
            self.dev[(L, n)] = tuple(self.g.to_device(np.ascontiguousarray(x[idx])) for x in self.operands(L))
        return self.dev[(L, n)]

    def expected(self, op, L, kind="uniform"):
        """[7, 2, L', N] by the oracle"""
        key = (op, L, kind)
        if key not in self.want:
            o = self.o
            A, B, C3 = self.operands(L)
            rk, gks = self.keys[kind]
            m = len(FAM)
            e1 = o.galois_elt(1)
            if op == "multiply_relin":
                w = [o.relinearize(o.multiply_ntt(A[i], B[i]), rk) for i in range(m)]
            elif op == "relinearize":
                w = [o.relinearize(C3[i], rk) for i in range(m)]
            elif op in ("multiply_relin_rescale", "relinearize_rescale"):
                w = [o.rescale(x) for x in self.expected(op[:-8], L, kind)]
            elif op == "rotate":
                w = [o.apply_galois(A[i], e1, gks[e1]) for i in range(m)]
            elif op == "rotate_add":
                w = [o.add(B[i], x) for i, x in enumerate(self.expected("rotate", L, kind))]
            elif op == "rotate_sum":
                w = []
                for i in range(m):
                    t = A[i].copy()
                    for s in lp.ROTATE_SUM_STEPS:
                        t = o.add(t, o.rotate(A[i], s, gks))
                    w.append(t)
            else:
                raise KeyError(op)
            self.want[key] = np.stack(w)
        return self.want[key]


class States:
    """one device context alive at a time (the cases are ordered by chain)"""

    def __init__(self, be, ho):
        self.be, self.ho, self.cur = be, ho, None

    def get(self, cid):
        if self.cur is None or self.cur.cid != cid:
            self.close()
            self.cur = State(self.be, self.ho, cid)
        return self.cur

    def close(self):
        if self.cur is not None:
            self.cur.close()
            self.cur = None


@pytest.fixture(scope="module")
def states(be, oracle):
    s = States(be, oracle)
    yield s
    s.close()
    print(f"paths wall time of the module: {time.time() - T0:.1f} s")


def batch_of(st, L, shape):
    """(n, chunk, LDS shape allowed) of a shape on this chain"""
    ch = st.chain
    if shape == "fused":
        n = next(n for n in range(1, 4097) if n % 8 and lp.ks_shape(ch, L, n, "product", True) == "fused")
        assert lp.ks_shape(ch, L, n - (n % 8), "product", True) != "fused" or n < 8
        return n, lp.DEFAULT_CHUNK, True
    n = min(5, lp.lat_limit(ch))
    if shape == "lds":
        assert lp.lds_shape(ch, L, 2)
        return n, 2, True
    return n, 2, False


def run_ks(st, op, L, shape, kind="uniform"):
    g, be, N = st.g, st.be, st.N
    n, chunk, lds = batch_of(st, L, shape)
    if op == "rotate_sum":
        chunk = lp.DEFAULT_CHUNK  # (the level walk cuts its own groups)
    st.use(kind)
    dA, dB, dC3 = st.slabs(L, n)
    want = st.expected(op, L, kind)
    rescale = op.endswith("rescale")
    Lo = L - 1 if rescale else L
    small = n <= 8
    out = sentinelled(g, n * 2 * Lo * N, N) if small else g.alloc(n * 2 * Lo * N)
    view = At(out, N) if small else out
    g.set_chunk(chunk)
    g.set_lds_max(None if lds else 0)
    try:
        g.sync()
        g.path_stats(reset=True)
        pw = be.Context.pairwise()
        if op.startswith("multiply_relin"):
            g.multiply_relin(L, n, dA, dB, pw, view, rescale=rescale)
        elif op == "relinearize":
            g.relinearize(L, n, dC3, view)
        elif op == "relinearize_rescale":
            g.relinearize_rescale(L, n, dC3, view)
        elif op == "rotate":
            g.rotate(L, n, dA, 1, view)
        elif op == "rotate_add":
            g.rotate_add(L, n, dA, 1, dB, view)
        else:
            g.rotate_sum(L, n, dA, list(lp.ROTATE_SUM_STEPS), view)
        g.sync()
        stats = g.path_stats()
        got = (inner_of(out, N, (st.cid, op, shape)) if small else out.download()).reshape(n, 2, Lo, N)
    finally:
        g.set_chunk(lp.DEFAULT_CHUNK)
        g.set_lds_max(None)
        out.free()
    what = f"{st.cid} {op} L = {L} {shape} n = {n} key {kind}"
    print(f"paths {what}: " + ", ".join(f"{k} = {v}" for k, v in stats.items() if v))
    if DEFAULT_SHAPES:
        plan = lp.plan_call(st.chain, PLAN_OP.get(op, op), L, n, chunk, key_steps=st.steps).counters()
        if not lds:
            plan["ks_latency"] += plan["ks_lds"]
            plan["ks_lds"] = 0
        assert {k: stats[k] for k in lp.COUNTERS} == plan, (what, stats, plan)
        if op != "rotate_sum":
            assert stats["ks_" + shape] >= 1 and sum(stats["ks_" + s] for s in ("lds", "latency", "unfused", "fused")) == stats["ks_" + shape], (what, stats)
    m = len(FAM)
    for r in range(n):
        if not np.array_equal(got[r], want[r % m]):
            same(got[r], want[r % m], f"{what}, row {r} ({FAM[r % m] or 'uniform'})")
    return stats


def ks_cases():
    return [(cid, L, op, shape) for cid in CKKS for L in levels(cid) for op in KS_OPS for shape in shapes(cid, L)]


@pytest.mark.parametrize("cid,L,op,shape", ks_cases(), ids=[f"{c}-L{L}-{op}-{s}" for c, L, op, s in ks_cases()])
def test_key_switch_matches_oracle(states, cid, L, op, shape):
    run_ks(states.get(cid), op, L, shape)


def key_cases():
    return [(cid, kind, op) for cid in CKKS for kind in KEY_KINDS for op in KEY_OPS]


@pytest.mark.parametrize("cid,kind,op", key_cases(), ids=["-".join(c) for c in key_cases()])
def test_key_switch_under_extreme_keys(states, cid, kind, op):
    """all-(q - 1) keys and the identity on the first / last digit, at the top level, in every shape; the identity keys against the closed
    form in Python integers as well as the oracle.  xbound_*: the all-(q - 1) keys one level below the top as well (terms == acc_terms)"""
    st = states.get(cid)
    L = st.o.L
    st.use(kind)
    if kind == "qm1":
        for Lp in levels(cid)[:-1]:
            for shape in shapes(cid, Lp):
                run_ks(st, op, Lp, shape, kind)
    if kind.startswith("identity"):
        A, B, C3 = st.operands(L)
        ops = eo.IdentityOps(st.o, st.j0(kind))
        want = st.expected(op, L, kind)
        for i in (0, 3, WORST_ROW):
            if op == "relinearize":
                closed = ops.relinearize(C3[i])
            elif op == "rotate":
                closed = ops.apply_galois(A[i], st.o.galois_elt(1))
            else:
                closed = st.o.rescale(ops.relinearize(st.o.multiply_ntt(A[i], B[i])))
            same(want[i], closed, f"{cid} {kind} {op}: the oracle against the closed form, row {i}")
    for shape in shapes(cid, L):
        run_ks(st, op, L, shape, kind)


@pytest.mark.parametrize("cid", [c for c in CKKS if c.startswith("xbound")])
def test_level_sums_inside_k3_on_both_sides_of_the_x_bound(states, cid):
    st = states.get(cid)
    g, N, m = st.g, st.N, len(FAM)
    for L in levels(cid):
        n = next(n for n in range(8, 4097, 8) if lp.level_sum_pays(st.chain, L, n))
        st.use("uniform")
        want = st.expected("rotate_sum", L)
        dA = st.slabs(L, n)[0]
        out = g.alloc(n * 2 * L * N)
        g.sync()
        g.path_stats(reset=True)
        g.rotate_sum(L, n, dA, list(lp.ROTATE_SUM_STEPS), out)
        g.sync()
        stats = g.path_stats()
        got = out.download((n, 2, L, N))
        out.free()
        print(f"paths {cid} rotate_sum L = {L} n = {n}, level sums: " + ", ".join(f"{k} = {v}" for k, v in stats.items() if v))
        if DEFAULT_SHAPES:
            assert stats["level_sums_in_k3"] >= 1 and stats["ks_fused"] >= 1 and stats["ks_lds"] == stats["ks_latency"] == stats["ks_unfused"] == 0, (cid, L, stats)
        for r in range(n):
            if not np.array_equal(got[r], want[r % m]):
                same(got[r], want[r % m], f"{cid} rotate_sum with level sums in k_k3, L = {L}, row {r}")


@pytest.mark.parametrize("cid", CKKS)
def test_elementwise_ops_match_oracle(states, cid):
    st = states.get(cid)
    g, o, be, N, rng = st.g, st.o, st.be, st.N, st.rng
    pw = be.Context.pairwise()
    for L in levels(cid):
        A, B, C3 = st.operands(L)
        n = 5
        dA, dB, dC3 = st.slabs(L, n)
        g.set_chunk(2)
        try:
            out3 = g.alloc(n * 3 * L * N)
            g.multiply(L, n, dA, dB, pw, out3)
            same(out3.download((n, 3, L, N)), C3[:n] if st.worst is None else np.stack([o.multiply_ntt(A[i], B[i]) for i in range(n)]), f"{cid} multiply L = {L}")
            pts = eo.batch(o, ["qm1", None, "half1", "planted", "alt_half"], L, 1, rng)[:, 0]
            out2 = g.alloc(n * 2 * L * N)
            g.multiply_plain(L, 2, n, dA, g.to_device(pts), pw, out2)
            same(out2.download((n, 2, L, N)), np.stack([o.multiply_plain(A[r], pts[r]) for r in range(n)]), f"{cid} multiply_plain L = {L}")
            if L > 1:
                for size, src, d in ((2, A, dA), (3, C3, dC3)):
                    lo = g.alloc(n * size * (L - 1) * N)
                    g.rescale(L, size, n, d, lo)
                    same(lo.download((n, size, L - 1, N)), np.stack([o.rescale(src[r]) for r in range(n)]), f"{cid} rescale size {size} L = {L}")
                for L_to in sorted({1, L - 1}):
                    lo = g.alloc(n * 2 * L_to * N)
                    g.mod_switch_drop(L, L_to, n * 2, dA, lo)
                    same(lo.download((n, 2, L_to, N)), np.stack([o.mod_switch_drop(A[r], L_to) for r in range(n)]), f"{cid} mod_switch_drop {L} -> {L_to}")
            inner = 33
            allq = eo.batch(o, ["qm1"] * inner, L, 2, rng)
            ma = np.concatenate([allq, eo.batch(o, [None] * inner, L, 2, rng)])
            d3 = g.alloc(2 * 3 * L * N)
            g.multiply_accumulate(L, 2, 1, inner, g.to_device(ma), inner, 1, g.to_device(allq), 1, 1, d3)
            got = d3.download((2, 3, L, N))
            for i in range(2):
                acc = o.multiply_ntt(ma[i * inner], allq[0])
                for k in range(1, inner):
                    acc = o.add(acc, o.multiply_ntt(ma[i * inner + k], allq[k]))
                same(got[i], acc, f"{cid} multiply_accumulate of 33 terms, row {i}, L = {L}")
            # the transforms, every prime of the level: forward of coefficient-form rows, inverse back
            coef = np.stack([np.stack([np.stack([o.intt(i, A[r, k, i]) for i in range(L)]) for k in range(2)]) for r in range(n)])
            buf = g.to_device(coef)
            g.ntt(buf, n * 2 * L, list(range(L)))
            same(buf.download(coef.shape), A[:n], f"{cid} ntt_forward L = {L}")
            g.ntt(buf, n * 2 * L, list(range(L)), inverse=True)
            same(buf.download(coef.shape), coef, f"{cid} ntt_inverse L = {L}")
        finally:
            g.set_chunk(lp.DEFAULT_CHUNK)
    # the special prime's transforms too
    K = len(st.primes)
    x = rng.integers(0, st.primes[-1], (3, N), dtype=np.uint64)
    x[1] = st.primes[-1] - 1
    buf = g.to_device(x)
    g.ntt(buf, 3, [K - 1])
    same(buf.download(x.shape), np.stack([o.ntt(K - 1, r) for r in x]), f"{cid} ntt_forward, special prime")
    g.ntt(buf, 3, [K - 1], inverse=True)
    same(buf.download(x.shape), x, f"{cid} ntt_inverse, special prime")


# ---- BFV ---------------------------------------------------------------------------------------------------------------------------------
def delta(o, m, L):
    """[L][N]: floor((q_L m + floor((t + 1) / 2)) / t) mod q_i in Python integers"""
    t, qs = o.t, o.moduli[:L]
    qL = co.prod(qs)
    d = (qL * m.astype(object) + (t + 1) // 2) // t
    return np.stack([(d % q).astype(np.uint64) for q in qs])


def edge_plains(t, n, N, rng):
    m = rng.integers(0, t, (n, N), dtype=np.uint64)
    edges = [0, 1, t // 2, min(t - 1, t // 2 + 1), t - 1]
    for r in range(n):
        m[r, r:r + 5] = edges
    m[n - 1] = t - 1
    return m


@pytest.mark.parametrize("cid", BFV)
def test_bfv_twin(be, oracle, cid):
    c = CH[cid]
    g, o, N, sk, pk = pair(be, oracle, (c["N"], c["primes"], c["t"]), keys=True)
    try:
        _bfv_twin(be, oracle, cid, c, g, o, N, sk, pk)
    finally:
        g.close()


def _bfv_twin(be, oracle, cid, c, g, o, N, sk, pk):
    t, L = c["t"], g.L
    assert g.moduli == c["primes"] and g.t == t and g.fp64 == [xm.is_f64(q) for q in c["primes"]]
    assert set(g.bfv_aux_base()).isdisjoint(c["primes"])
    rng = np.random.default_rng(t % 9973 + L)
    pw = be.Context.pairwise()
    n = 4
    m = edge_plains(t, n, N, rng)
    dm = g.to_device(m)
    # encrypt: the oracle driven with the polynomials the device sampled
    seed, first = 0xC0FFEE, 40
    cts = g.alloc(n * 2 * L * N)
    g.encrypt(n, dm, seed, first, cts)
    enc = cts.download((n, 2, L, N))
    for r in range(n):
        su, s0, s1 = sn.enc_streams(first + r)
        same(enc[r], o.encrypt_explicit(pk, m[r], sn.sample_ternary(seed, su, N), sn.sample_cbd(seed, s0, N), sn.sample_cbd(seed, s1, N)), f"{cid} encrypt {r}")
    # decrypt: the encryptions, and phases planted on both sides of the rounding's tie points at every level
    dec = g.alloc(n * N)
    g.decrypt(L, 2, n, cts, dec)
    same(dec.download((n, N)), m, f"{cid} decrypt(encrypt)")
    for Lp in sorted({1, L}):
        qs = o.moduli[:Lp]
        Q = co.prod(qs)
        phases = co.phase_batch(Q, t, N, n)
        pc = np.stack([co.bfv_ct_with_phase(phases[r], qs, 2, "zero", rng) for r in range(n)])
        dp = g.to_device(pc)
        g.decrypt(Lp, 2, n, dp, dec)
        got = dec.download((n, N))
        for r in range(n):
            same(got[r], o.bfv_decode_phase(o.decrypt_phase(pc[r], sk)), f"{cid} decrypt of planted phases, L = {Lp}, row {r}")
            assert [int(v) for v in got[r]] == [co.bfv_round_closed_form(x, Q, t) for x in phases[r]], (cid, Lp, r, "the closed form of the rounding")
    # the BEHZ multiply on the operand families, relinearized
    fam = family_cts(o, L, N) + [o.random_poly(rng, L, 2) for _ in range(2)] + [enc[0], enc[n - 1]]
    pairs = [(0, 0), (1, 2), (3, 1), (4, 6), (5, 4), (7, 8), (9, 10), (10, 10)]
    a = np.stack([fam[i] for i, _ in pairs])
    b = np.stack([fam[j] for _, j in pairs])
    rk = o.keygen_relin(sk, 23)
    g.set_relin_key(rk)
    c3, c2 = g.alloc(len(pairs) * 3 * L * N), g.alloc(len(pairs) * 2 * L * N)
    g.bfv_multiply(L, len(pairs), g.to_device(a), g.to_device(b), pw, c3)
    g.relinearize(L, len(pairs), c3, c2)
    got3, got2 = c3.download((len(pairs), 3, L, N)), c2.download((len(pairs), 2, L, N))
    prods = [o.bfv_multiply(a[r], b[r]) for r in range(len(pairs))]
    for r in range(len(pairs)):
        same(got3[r], prods[r], f"{cid} bfv_multiply, pair {pairs[r]}")
        same(got2[r], o.relinearize(prods[r], rk), f"{cid} bfv_multiply + relinearize, pair {pairs[r]}")
    sq = got2[len(pairs) - 1]
    # the fused multiply -> relinearize -> add: result j = sum_k a(k) b(k, j), 2 results of 3 terms (b(k, j) at k * 2 + j)
    ka, kb = [1, 7, 9], [[2, 8], [4, 3], [10, 6]]
    A3 = np.stack([fam[i] for i in ka])
    B3 = np.stack([fam[j] for row in kb for j in row])
    fused = g.alloc(2 * 2 * L * N)
    g.bfv_multiply_relin_accumulate(L, 1, 2, 3, g.to_device(A3), 3, 1, g.to_device(B3), 2, 1, fused)
    gotf = fused.download((2, 2, L, N))
    for j in range(2):
        acc = np.zeros((2, L, N), dtype=object)
        for k in range(3):
            acc = acc + o.relinearize(o.bfv_multiply(fam[ka[k]], fam[kb[k][j]]), rk).astype(object)
        want = np.stack([np.stack([acc[p2][i] % int(q) for i, q in enumerate(o.moduli[:L])]) for p2 in range(2)]).astype(np.uint64)
        same(gotf[j], want, f"{cid} bfv_multiply_relin_accumulate, result {j}")
    # the noise budget: fresh encryptions, a product, uniform rows
    rows = np.concatenate([enc, got2[-2:], np.stack([o.random_poly(rng, L, 2)])])
    budget, bits = g.bfv_noise_budget(L, 2, len(rows), g.to_device(rows), with_bits=True)
    want = [noise.noise_of(o, ct, sk) for ct in rows]
    print(f"paths {cid} noise budget: {budget.tolist()}")
    assert bits.tolist() == [w[0] for w in want] and budget.tolist() == [w[1] for w in want], (cid, bits, budget, want)
    assert budget[0] > 0 and budget[-1] == 0
    g.decrypt(L, 2, 1, g.to_device(sq[None]), dec)  # (a product of two encryptions: whatever budget it has left, the same rounding)
    same(dec.download((n, N))[0], o.bfv_decode_phase(o.decrypt_phase(sq, sk)), f"{cid} decrypt of a relinearized product")
    # mod_switch, add_plain / sub_plain, multiply_plain at the top level and one below
    for Lp in sorted({L, max(1, L - 1)}):
        x = np.stack([o.random_poly(rng, Lp, 2) for _ in range(n)])
        x[0] = eo.family(o, "qm1", Lp, 2, coeff_form=True)
        x[1] = eo.family(o, "planted", Lp, 2, rng, coeff_form=True)
        dx = g.to_device(x)
        for L_to in sorted({1, Lp - 1} - {0, Lp}):
            lo = g.alloc(n * 2 * L_to * N)
            g.bfv_mod_switch(Lp, L_to, 2, n, dx, lo)
            want = []
            for r in range(n):
                w = x[r]
                while w.shape[1] > L_to:
                    w = o.mod_switch_coeff(w)
                want.append(w)
            same(lo.download((n, 2, L_to, N)), np.stack(want), f"{cid} bfv_mod_switch {Lp} -> {L_to}")
        out = g.alloc(n * 2 * Lp * N)
        for sub in (False, True):
            g.bfv_add_plain(Lp, 2, n, dx, dm, pw, out, sub=sub)
            got = out.download((n, 2, Lp, N))
            for r in range(n):
                d = delta(o, m[r], Lp)
                w = x[r].copy()
                for i, q in enumerate(o.moduli[:Lp]):
                    w[0, i] = ((x[r, 0, i].astype(object) + (-1 if sub else 1) * d[i].astype(object)) % q).astype(np.uint64)
                same(got[r], w, f"{cid} bfv_{'sub' if sub else 'add'}_plain L = {Lp}, row {r}")
        g.bfv_multiply_plain(Lp, 2, n, dx, dm, pw, out)
        got = out.download((n, 2, Lp, N))
        lifted = [lift(o, m[r], Lp) for r in range(n)]
        for r in range(n):
            w = np.empty_like(x[r])
            for i, q in enumerate(o.moduli[:Lp]):
                pm = o.ntt(i, lifted[r][i]).astype(object)
                for k in range(2):
                    w[k, i] = o.intt(i, ((o.ntt(i, x[r, k, i]).astype(object) * pm) % q).astype(np.uint64))
            same(got[r], w, f"{cid} bfv_multiply_plain L = {Lp}, row {r}")
        # plain_to_ntt: the centred lift under every prime (the threshold (t + 1) / 2)
        pn = g.alloc(n * Lp * N)
        g.bfv_plain_to_ntt(Lp, n, dm, pn)
        same(pn.download((n, Lp, N)), np.stack([np.stack([o.ntt(i, lifted[r][i]) for i in range(Lp)]) for r in range(n)]), f"{cid} bfv_plain_to_ntt L = {Lp}")
    # multiply_plain_accumulate over more terms than the shortest run of the level: every term (q - 1)^2, beside a uniform result
    run = min(xm.mac_run(q) for q in o.moduli[:L])
    inner = run + 1 if run <= 1024 else 5
    ct = np.empty((2, inner, 2, L, N), dtype=np.uint64)
    pt = np.empty((inner, L, N), dtype=np.uint64)
    for i, q in enumerate(o.moduli[:L]):
        ct[0, :, :, i] = q - 1
        ct[1, :, :, i] = rng.integers(0, q, (inner, 2, N), dtype=np.uint64)
        pt[:, i] = q - 1
        pt[inner // 2:, i, 1::2] = rng.integers(0, q, (inner - inner // 2, N // 2), dtype=np.uint64)
    acc = g.alloc(2 * 2 * L * N)
    g.bfv_multiply_plain_accumulate(L, 2, 2, 1, inner, g.to_device(ct), inner, 1, g.to_device(pt), 1, 1, acc)
    got = acc.download((2, 2, L, N))
    cols = list(range(40)) + list(range(1000, 1040)) + [N - 2, N - 1]  # Python integers on these columns; the closed form on the rest
    for i, q in enumerate(o.moduli[:L]):
        w = (ct[:, :, :, i][..., cols].astype(object) * pt[None, :, None, i][..., cols].astype(object)).sum(axis=1) % q
        same(got[:, :, i][..., cols], w.astype(np.uint64), f"{cid} bfv_multiply_plain_accumulate over {inner} terms (run {run}), prime {i}")
        assert (got[0, :, i, 0::2] == np.uint64(inner % q)).all(), (cid, i, "every term (q - 1)^2 = 1 (mod q): the sum is the number of terms")
    # the batch encoder needs t = 1 (mod 2N), t prime: refused elsewhere with the message of he355_bfv_encode
    vals = rng.integers(-(t // 2), t // 2 + 1, (2, N)).astype(np.int64)
    dv, plain, back = g.to_device(vals.view(np.uint64)), g.alloc(2 * N), g.alloc(2 * N)
    if c["batching"]:
        codec = oracle.BatchCodec(N, t)
        g.bfv_encode(2, dv, N, plain)
        same(plain.download((2, N)), np.stack([codec.encode(v) for v in vals]), f"{cid} bfv_encode")
        g.bfv_decode(2, plain, back)
        assert np.array_equal(back.download().view(np.int64).reshape(2, N) % t, vals % t), (cid, "bfv_decode")
    else:
        for call in (lambda: g.bfv_encode(2, dv, N, plain), lambda: g.bfv_decode(2, plain, back)):
            with pytest.raises(be.HE355Error) as ei:
                call()
            assert ei.value.code == be.E_INVALID_ARGS and "batching plain modulus" in str(ei.value), ei.value
        refused(be, lambda: g.bfv_encode(2, dv, N, plain))
