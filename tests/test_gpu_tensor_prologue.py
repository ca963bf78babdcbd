"""The ct x ct prologue of the fused key product (k_k3<TENSOR>: c0, c1, c2 from three products of one load of each operand row, c2
handed to the own digit's key product) and k_k1<K1_MUL_C2>'s operand loads ahead of its twiddle staging, held to the oracle bit for
bit (run with -m gpu on an MI355X).

Chains: {60,40,40,60} at N = 4096 and {60,45,45,60} at N = 2^15 (L = 3): both engines' TENSOR instantiations run, fused and raw tail.
Batches, from tests/launch_plan.py: the smallest that takes the fused throughput shape (249 / 25: ragged, the last op-group holds one
ciphertext of eight), and the smallest whose data-prime launch runs two op-groups per block with an odd number of op-groups (257 / 33
without rescale, 513 / 65 with it): its blocks run a second op-group behind the first, and its last block has no second one.  Each
batch runs twice in one process with the other in between.

Operands: result r = i * nb + x multiplies a[i] and b[x] (the outer indexer).  The a rows cycle through uniform, every residue q - 1,
a ciphertext whose two polynomials are equal (a0 = a1), uniform; b is ONE ciphertext (every residue q - 1) or three (uniform, q - 1,
uniform: idx_b changes inside every block).  The oracle computes the twelve distinct products once per chain.  The output lies between
two ciphertexts of sentinel words and is itself filled with them; the operands are read back and compared afterwards.

k_k1: multiply + relinearize (size-3 output, then K1_CT3 and the plain fused k_k3), multiply_relin with `out` apart (k_k1<K1_MUL_C2>, in
every case above: asserted from the plan) and multiply_relin with `out` laid over operand a at a batch beyond the dual launch's grid
(k_k1<K1_MUL>, both engines' own launches)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edge_operands as eo  # noqa: E402
import launch_plan as lp  # noqa: E402
from bfv_gpu_helpers import SENT  # noqa: E402

_SHAPE_ENV = ("HE355_CHUNK", "HE355_LATENCY_MAX", "HE355_LEVEL_WALK", "HE355_LDS_MAX", "HE355_FORCE_U64")
DEFAULT_SHAPES = not any(os.environ.get(k) for k in _SHAPE_ENV)
# name -> (N, bit sizes, {rescale: (smallest fused batch, smallest batch with a partial last block)}, batch of the K1_MUL launch)
CHAINS = {
    "n4096_60_40_40_60": (4096, [60, 40, 40, 60], {False: (249, 257), True: (249, 513)}, 345),
    "n32768_60_45_45_60": (32768, [60, 45, 45, 60], {False: (25, 33), True: (25, 65)}, 45),
}
A_KINDS = ["uniform", "qm1", "equal_polys", "uniform"]
B_KINDS = ["uniform", "qm1", "uniform"]
NB_CASES = {"b_one": (1, 1), "b_three": (3, 0)}  # name -> (ciphertexts of b the indexer walks, b_base)


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need an MI355X (the backend has no CPU fallback)")
    return mod


class View:
    """a window of a device slab: what the Context methods take (`.ptr`)"""

    def __init__(self, buf, offset_u64):
        self.ptr = C.c_void_p(buf.ptr.value + int(offset_u64) * 8)


def data_prime_groups(ch, op, L, n):
    """(op-groups per block of the fp64 engine's data-prime k_k3 launch, op-groups) of one fused call"""
    plan = lp.plan_call(ch, op, L, n)
    assert [c.shape for c in plan.chunks] == ["fused"], (op, n)
    for l in plan.launches():
        if l.family == "k_k3_dual8" and "data primes" in l.note:
            return int(l.note.split("og_per_block")[1].split()[1]), -(-n // 8), plan
        if l.family == "k_k3" and "data primes" in l.note and l.engine == "fp64":
            return l.og_per_block, -(-n // 8), plan
    raise AssertionError("no data-prime k_k3 launch in the plan")


class State:
    def __init__(self, be, ho, name):
        N, bits, self.batches, self.n_k1 = CHAINS[name]
        self.name, self.N = name, N
        kw = dict(bit_sizes=list(bits), sec128=False)
        self.g = be.Context(be.SCHEME_CKKS, N, device=0, **kw)
        self.o = o = ho.Context(ho.SCHEME_CKKS, N, **kw)
        assert self.g.moduli == o.moduli
        self.L = L = self.g.L
        assert L == 3 and not all(self.g.fp64[:L]) and any(self.g.fp64[:L])  # both engines own data primes
        self.chain = ch = lp.chain("ckks", N, bits, self.g.fp64)
        for rescale, (n_min, n_part) in self.batches.items():
            op = "multiply_relin_rescale" if rescale else "multiply_relin"
            assert lp.ks_shape(ch, L, n_min, "product", True) == "fused" and lp.ks_shape(ch, L, n_min - 1, "product", True) != "fused" and n_min % 8
            assert n_min == min(n for n in lp.boundary_cases(ch, op, L, ("shape",)) if lp.ks_shape(ch, L, n, "product", True) == "fused")
            ogpb, n_og, plan = data_prime_groups(ch, op, L, n_part)
            assert ogpb == 2 and n_og % 2 == 1 and n_part % 8, (op, n_part)  # a second op-group per block, none in the last block
            for n in (n_min, n_part):  # `out` apart: k_k1 writes the key-switch target only (K1_MUL_C2), one launch per engine
                assert [l.family for l in lp.plan_call(ch, op, L, n).launches()][:2] == ["k_k1", "k_k1"], (op, n)
        rng = np.random.default_rng(sum(bits) * 977 + N)
        self.rk = o.random_kswitch_key(rng)
        self.g.set_relin_key(self.rk)
        self.A = np.stack([self._operand(k, rng) for k in A_KINDS])
        self.B = np.stack([self._operand(k, rng) for k in B_KINDS])
        self.c3, self.relin, self.resc = {}, {}, {}
        for i in range(len(A_KINDS)):
            for x in range(len(B_KINDS)):
                self.c3[i, x] = o.multiply_ntt(self.A[i], self.B[x])
                self.relin[i, x] = o.relinearize(self.c3[i, x], self.rk)
                self.resc[i, x] = o.rescale(self.relin[i, x])
        n_max = max(max(v) for v in self.batches.values())
        self.a_rows = np.ascontiguousarray(self.A[np.arange(n_max) % len(A_KINDS)])
        self.dA, self.dB = self.g.to_device(self.a_rows), self.g.to_device(self.B)

    def _operand(self, kind, rng):
        if kind == "qm1":
            return eo.family(self.o, "qm1", self.L, 2)
        p = self.o.random_poly(rng, self.L, 2)
        if kind == "equal_polys":
            p[1] = p[0]
        return p

    def close(self):
        self.g.close()


class States:
    def __init__(self, be, ho):
        self.be, self.ho, self.cur = be, ho, None

    def get(self, name):
        if self.cur is None or self.cur.name != name:
            self.close()
            self.cur = State(self.be, self.ho, name)
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


def _free(g, *bufs):
    for b in bufs:
        b.free()
        g._bufs.remove(b)


def _check_rows(what, got, want_of_row):
    for r in range(len(got)):
        want = want_of_row(r)
        if not np.array_equal(got[r], want):
            bad = np.argwhere(got[r] != want)
            raise AssertionError(what + (f"row {r} of {len(got)} differs from the oracle in {len(bad)} words, first at [poly, prime, coefficient] = {bad[0].tolist()}",))


def run_outer(st, be, n, nb, b_base, rescale, what):
    """multiply_relin over n results, r = i * nb + x from a[i], b[b_base + x], between sentinels; operands unchanged afterwards"""
    g, L, N = st.g, st.L, st.N
    Lo = L - 1 if rescale else L
    per = 2 * Lo * N
    slab = g.to_device(np.full((n + 2) * per, SENT, dtype=np.uint64))
    try:
        g.sync()
        g.path_stats(reset=True)
        g.multiply_relin(L, n, st.dA, st.dB, be.Context.outer(0, -(-n // nb), b_base, nb), View(slab, per), rescale=rescale)
        g.sync()
        stats = g.path_stats()
        flat = slab.download()
    finally:
        _free(g, slab)
    what = what + (f"n={n}",)
    if DEFAULT_SHAPES:
        assert stats["ks_fused"] == 1 and stats["ks_lds"] == stats["ks_latency"] == stats["ks_unfused"] == 0, what + (stats,)
    assert (flat[:per] == SENT).all(), what + ("the ciphertext of sentinel words BEFORE the output was written",)
    assert (flat[(n + 1) * per:] == SENT).all(), what + ("the ciphertext of sentinel words AFTER the output was written",)
    want = st.resc if rescale else st.relin
    _check_rows(what, flat[per:(n + 1) * per].reshape(n, 2, Lo, N), lambda r: want[(r // nb) % len(A_KINDS), b_base + r % nb])
    assert np.array_equal(st.dA.download(st.a_rows.shape), st.a_rows), what + ("operand a was changed",)
    assert np.array_equal(st.dB.download(st.B.shape), st.B), what + ("operand b was changed",)


@pytest.mark.parametrize("nb_case", list(NB_CASES))
@pytest.mark.parametrize("rescale", [False, True], ids=["relin", "relin_rescale"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_tensor_prologue_matches_oracle(be, states, name, rescale, nb_case):
    st = states.get(name)
    nb, b_base = NB_CASES[nb_case]
    n_min, n_part = st.batches[rescale]
    for n in (n_part, n_min, n_part, n_min):  # each batch twice, the other in between: a row left in a landing buffer would show
        run_outer(st, be, n, nb, b_base, rescale, (name, "rescale" if rescale else "no rescale", nb_case))


@pytest.mark.parametrize("name", list(CHAINS))
def test_multiply_then_relinearize_matches_oracle(be, states, name):
    """he355_multiply (size-3 output) + he355_relinearize at the smallest fused batch: K1_CT3 and the plain fused k_k3 beside the tensor path"""
    st = states.get(name)
    g, L, N = st.g, st.L, st.N
    n, nb = st.batches[False][0], 3
    c3, out = g.alloc(n * 3 * L * N), g.alloc(n * 2 * L * N)
    try:
        g.multiply(L, n, st.dA, st.dB, be.Context.outer(0, -(-n // nb), 0, nb), c3)
        g.relinearize(L, n, c3, out)
        g.sync()
        got3, got = c3.download((n, 3, L, N)), out.download((n, 2, L, N))
    finally:
        _free(g, c3, out)
    _check_rows((name, "multiply"), got3, lambda r: st.c3[(r // nb) % len(A_KINDS), r % nb])
    _check_rows((name, "multiply + relinearize"), got, lambda r: st.relin[(r // nb) % len(A_KINDS), r % nb])


@pytest.mark.parametrize("name", list(CHAINS))
def test_k1_mul_launch_matches_oracle(be, states, name):
    """multiply_relin with `out` laid over operand a, at a ragged batch whose k_k1 grid is beyond the both-engines launch: k_k1<K1_MUL>
    writes c0, c1 and the key-switch target, one launch per engine; pairwise operands, run twice"""
    st = states.get(name)
    g, L, N, n = st.g, st.L, st.N, st.n_k1
    plan = lp.plan_call(st.chain, "multiply_relin_over_a", L, n)
    assert [c.shape for c in plan.chunks] == ["fused"] and [l.family for l in plan.launches()][:2] == ["k_k1", "k_k1"] and n % 4
    per = 2 * L * N
    ia, ib = np.arange(n) % len(A_KINDS), np.arange(n) % len(B_KINDS)
    b_rows = np.ascontiguousarray(st.B[ib])
    db = g.to_device(b_rows)
    try:
        for rep in range(2):
            host = np.concatenate([np.full(per, SENT, dtype=np.uint64), st.A[ia].reshape(-1), np.full(per, SENT, dtype=np.uint64)])
            slab = g.to_device(host)
            try:
                g.sync()
                g.path_stats(reset=True)
                g.multiply_relin(L, n, View(slab, per), db, be.Context.pairwise(), View(slab, per))
                g.sync()
                stats = g.path_stats()
                flat = slab.download()
            finally:
                _free(g, slab)
            what = (name, "out over a", f"n={n}", f"run {rep}")
            if DEFAULT_SHAPES:
                assert stats["ks_fused"] == 1 and stats["ks_lds"] == stats["ks_latency"] == stats["ks_unfused"] == 0, what + (stats,)
            assert (flat[:per] == SENT).all() and (flat[(n + 1) * per:] == SENT).all(), what + ("a ciphertext of sentinel words beside the slab was written",)
            _check_rows(what, flat[per:(n + 1) * per].reshape(n, 2, L, N), lambda r: st.relin[int(ia[r]), int(ib[r])])
            assert np.array_equal(db.download(b_rows.shape), b_rows), what + ("operand b was changed",)
    finally:
        _free(g, db)
