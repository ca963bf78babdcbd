"""The fused key switch's floor steps, own digit and raw tail on the fp64 engine, held to the oracle bit for bit on chains on both sides of
the host-side bound of the direct floor forms (csrc/modarith.h: floor_direct_terms; run with -m gpu on an MI355X).

  * {47,46,45,44,47}: the 47- and 46-bit targets are beyond the bound (sums and correction rows are re-centred first), the 45- and
    44-bit ones inside it -- both ways in one launch;
  * {60,45 x 7,60}: L = 8, every fp64 target takes the direct forms with ten terms per sum, under a relinearization key whose every
    residue is q_t - 1;
  * {60,40,40,60} at N = 2^15.

multiply_relin with and without rescale runs the TENSOR instantiations (floor_fin_s_acc / floor_fin2_s_acc, the own digit as a lazy
product, the raw tail with its re-centred sums); relinearize of size 3 and the two rotations run k_k3<FUSE,!TENSOR,!GROUPED>, which
keeps the canonical forms (csrc/k3_body.inc: kAccForms) and is held here to the same oracle beside them.  rotate_sum with the level
sums formed inside k_k3 (asserted: level_sums_in_k3) runs the GROUPED instantiation, where floor_fin_acc reads the double sums: on
{47,46,45,44,47} behind floor_prep for two of the four targets, on the 45-bit chain directly.  (floor_fin2_acc has no caller on the
device today -- no grouped launch rescales -- and is held by tests/test_floor_forms_cpu.py alone.)

Which targets re-centre first is the host-side rule floor_direct_terms; tests/test_floor_forms_cpu.py holds that rule, and the forms on
both sides of it, to Python integers.  Nothing here can tell the two branches apart on the device: both are exact for these chains'
magnitudes, so this module checks that each branch the rule selects computes the oracle's bits, not which branch ran.

Batches are the smallest ragged ones that take the fused throughput shape (fuse_pays: 128 special-prime blocks -- 32 op-groups at
N = 4096, 4 at N = 32768; the last op-group holds 3 of 8), asserted with he355_path_stats.  Row r holds operand pair r mod 7: four
uniform pairs and the `qm1`, `qm1_coeff` and `planted` families of tests/edge_operands.py; the oracle computes the seven once per chain."""
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
import shoup_rings as shoup  # noqa: E402

_SHAPE_ENV = ("HE355_CHUNK", "HE355_LATENCY_MAX", "HE355_LEVEL_WALK", "HE355_LDS_MAX", "HE355_FORCE_U64")
DEFAULT_SHAPES = not any(os.environ.get(k) for k in _SHAPE_ENV)
FAMILIES = [None, None, None, None, "qm1", "qm1_coeff", "planted"]
# name -> (N, bit sizes, batch, relinearization key kind)
CHAINS = {
    "n4096_47_46_45_44_47": (4096, [47, 46, 45, 44, 47], 251, "uniform"),
    "n4096_60_45x7_60": (4096, [60] + [45] * 7 + [60], 251, "qm1"),
    "n32768_60_40_40_60": (32768, [60, 40, 40, 60], 27, "uniform"),
    # the Shoup build at LOGN1 = 4 (tests/shoup_rings.py): its fp64 prime's floor forms beside a 60- and a 50-bit prime of the u64 engine
    "n16384_60_50_40_60_shoup": (16384, [60, 50, 40, 60], 59, "uniform"),
}
OPS = ["multiply_relin", "multiply_relin_rescale", "relinearize", "relinearize_rescale", "rotate", "rotate_add"]
# rotate_sum with the level sums inside k_k3 (level_sum_pays: whole groups of eight, 512 blocks in the data-prime launch): chain -> batch
SUM_BATCH = {"n4096_47_46_45_44_47": 256, "n4096_60_45x7_60": 256, "n32768_60_40_40_60": 48, "n16384_60_50_40_60_shoup": 88}


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need an MI355X (the backend has no CPU fallback)")
    return mod


class State:
    def __init__(self, be, ho, name):
        N, bits, n, key_kind = CHAINS[name]
        self.name, self.N, self.n = name, N, n
        kw = dict(bit_sizes=list(bits), sec128=False)
        self.g = be.Context(be.SCHEME_CKKS, N, device=0, **kw)
        self.o = o = ho.Context(ho.SCHEME_CKKS, N, **kw)
        assert self.g.moduli == o.moduli
        if name in shoup.RINGS:
            shoup.check_device(name, self.g)
        self.L = L = self.g.L
        self.chain = lp.chain("ckks", N, bits, self.g.fp64)
        assert lp.ks_shape(self.chain, L, n, "product", True) == "fused" and lp.ks_shape(self.chain, L, n - 8, "product", True) != "fused" and n % 8
        rng = np.random.default_rng(sum(bits) * 131 + N)
        self.rk = eo.key(o, key_kind, rng)
        self.g.set_relin_key(self.rk)
        self.elt = o.galois_elt(1)
        self.gks = {o.galois_elt(s): eo.key(o, "uniform", rng) for s in lp.ROTATE_KEY_STEPS}
        for e, k in self.gks.items():
            self.g.set_galois_key(e, k)
        self.gk = self.gks[self.elt]
        m = len(FAMILIES)
        self.A = eo.batch(o, FAMILIES, L, 2, rng)
        self.B = eo.batch(o, FAMILIES[::-1], L, 2, rng)  # (the families meet uniform partners, and each other in the middle)
        self.C3 = np.stack([o.multiply_ntt(self.A[i], self.B[i]) for i in range(m)])
        idx = np.arange(n) % m
        self.dA, self.dB, self.dC3 = (self.g.to_device(np.ascontiguousarray(x[idx])) for x in (self.A, self.B, self.C3))
        relin = np.stack([o.relinearize(self.C3[i], self.rk) for i in range(m)])
        rot = np.stack([o.apply_galois(self.A[i], self.elt, self.gk) for i in range(m)])
        self.want = {
            "multiply_relin": relin, "relinearize": relin,
            "multiply_relin_rescale": np.stack([o.rescale(x) for x in relin]),
            "rotate": rot, "rotate_add": np.stack([o.add(self.B[i], rot[i]) for i in range(m)]),
        }
        self.want["relinearize_rescale"] = self.want["multiply_relin_rescale"]

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


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", list(CHAINS))
def test_fused_key_switch_matches_oracle(states, name, op):
    st = states.get(name)
    g, L, n, N = st.g, st.L, st.n, st.N
    rescale = op.endswith("rescale")
    Lo = L - 1 if rescale else L
    out = g.alloc(n * 2 * Lo * N)
    try:
        g.sync()
        g.path_stats(reset=True)
        if op.startswith("multiply_relin"):
            g.multiply_relin(L, n, st.dA, st.dB, type(g).pairwise(), out, rescale=rescale)
        elif op == "relinearize":
            g.relinearize(L, n, st.dC3, out)
        elif op == "relinearize_rescale":
            g.relinearize_rescale(L, n, st.dC3, out)
        elif op == "rotate":
            g.rotate(L, n, st.dA, 1, out)
        else:
            g.rotate_add(L, n, st.dA, 1, st.dB, out)
        g.sync()
        stats = g.path_stats()
        got = out.download((n, 2, Lo, N))
    finally:
        out.free()
        g._bufs.remove(out)
    if DEFAULT_SHAPES:
        assert stats["ks_fused"] >= 1 and stats["ks_lds"] == stats["ks_latency"] == stats["ks_unfused"] == 0, (name, op, stats)
    want, m = st.want[op], len(FAMILIES)
    for r in range(n):
        if not np.array_equal(got[r], want[r % m]):
            bad = np.argwhere(got[r] != want[r % m])
            raise AssertionError((name, op, f"row {r} of {n} ({FAMILIES[r % m] or 'uniform'}) differs from the oracle in {len(bad)} words, first at "
                                             f"[poly, prime, coefficient] = {bad[0].tolist()}"))


@pytest.mark.parametrize("name", list(SUM_BATCH))
def test_grouped_level_sums_match_oracle(states, name):
    """out = a + sum of three rotations, every level's sum formed by the fused grouped k_k3 (floor_fin_acc with the sum's row in the addend)"""
    st = states.get(name)
    g, o, L, N, n, m = st.g, st.o, st.L, st.N, SUM_BATCH[name], len(FAMILIES)
    assert lp.level_sum_pays(st.chain, L, n) and n % 8 == 0
    want = []
    for i in range(m):
        t = st.A[i].copy()
        for s in lp.ROTATE_SUM_STEPS:
            t = o.add(t, o.rotate(st.A[i], s, st.gks))
        want.append(t)
    da = g.to_device(np.ascontiguousarray(st.A[np.arange(n) % m]))
    out = g.alloc(n * 2 * L * N)
    try:
        g.sync()
        g.path_stats(reset=True)
        g.rotate_sum(L, n, da, list(lp.ROTATE_SUM_STEPS), out)
        g.sync()
        stats = g.path_stats()
        got = out.download((n, 2, L, N))
    finally:
        for b in (out, da):
            b.free()
            g._bufs.remove(b)
    if DEFAULT_SHAPES:
        assert stats["level_sums_in_k3"] >= 1 and stats["ks_fused"] >= 1 and stats["ks_lds"] == stats["ks_latency"] == stats["ks_unfused"] == 0, (name, stats)
    for r in range(n):
        assert np.array_equal(got[r], want[r % m]), (name, f"row {r} of {n} ({FAMILIES[r % m] or 'uniform'}) differs from the oracle")
