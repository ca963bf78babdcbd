"""Key switches held to the oracle on both sides of every kernel-selection boundary (run with -m gpu on an MI355X).

The library picks a kernel sequence per chunk (ks_shape: ring-in-LDS, latency, unfused, fused) and a grid per launch (one launch for both
engines or one each, the target split of k_k2n, op-groups per block and waves of k_k3, the level sum's grid) from the batch size, the
ring, the level and the engine of each prime.  Every one of those choices changes which rows a block owns and where the last, partly
filled op-group ends.  tests/launch_plan.py restates the rules; `boundary_cases` derives from them, per (chain, op), the smallest batch
on each side of every decision and the batches around the next multiple of 8.  This module runs those batches under the library's OWN
rule -- set_latency_max(None), set_lds_max(None), the default chunk -- and

  * compares EVERY result row with the oracle (np.array_equal).  The batch tiles 7 distinct ciphertext pairs (row r holds pair r mod 7,
    each row stored separately on the device), its last 8 rows are 8 further pairs, and the very last row is the `qm1` family
    (tests/edge_operands.py) under a uniform key: at most 15 oracle results per (chain, op), computed once per chain;
  * allocates the output between one ciphertext of sentinel words before it and one after it, both untouched afterwards, and fills the
    output itself with the sentinel, so a row that no block wrote shows as well as a row written past the slab;
  * downloads the operands after the call and compares them with what was uploaded;
  * walks the batch sizes of a case upwards and downwards within one context, so that each runs once directly after a smaller and once
    directly after a larger one (stale scratch of the previous plan), he355_path_stats reset per call;
  * asserts the shape and level-sum counters of he355_path_stats against the plan (only under the library's default settings, as
    tests/test_gpu_bench_shapes.py does: under tools/test_matrix.sh's settings the bits alone are held).

The mixed-shape calls cut a batch so that the body chunks take a throughput shape and the ragged last chunk the LDS or the latency
shape, with the two-stream schedule on and off; the counters must show both shapes in the one call.

With HE355_PLAN_LOG=<file> every call appends its planned launches as a JSON line: tools/plan_vs_trace.py compares them with a
rocprofv3 kernel trace of this module (profiles/selection_boundaries.txt)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import edge_operands as eo  # noqa: E402
import launch_plan as lp  # noqa: E402
import shoup_rings as sr  # noqa: E402
from bfv_gpu_helpers import SENT  # noqa: E402

# (tests/test_gpu_bench_shapes.py) the counter assertions describe the library's own choice of shape
_SHAPE_ENV = ("HE355_CHUNK", "HE355_LATENCY_MAX", "HE355_LEVEL_WALK", "HE355_LDS_MAX", "HE355_FORCE_U64")
DEFAULT_SHAPES = not any(os.environ.get(k) for k in _SHAPE_ENV)
PLAN_LOG = os.environ.get("HE355_PLAN_LOG")
N_TILE, N_TAIL = 7, 8  # row r holds pair r mod 7; the last 8 rows hold pairs 7 .. 14


@pytest.fixture(scope="module")
def be():
    mod = importlib.import_module("reference-seal-backend_amd")
    if mod.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need an MI355X (the backend has no CPU fallback)")
    return mod


def pair_of_rows(n):
    """which of the 15 distinct pairs each of the n rows holds"""
    idx = np.arange(n) % N_TILE
    k = min(n, N_TAIL)
    idx[n - k:] = np.arange(N_TILE + N_TAIL - k, N_TILE + N_TAIL)
    return idx


class View:
    """a window of a device slab: what the Context methods take (`.ptr`)"""

    def __init__(self, buf, offset_u64, n_u64):
        self.ptr, self.n = C.c_void_p(buf.ptr.value + int(offset_u64) * 8), int(n_u64)


class ChainState:
    """one chain's device and oracle contexts, keys, the 15 distinct operand pairs per level (host and device) and the oracle's results"""

    def __init__(self, be, ho, name, rot_steps):
        self.be, self.ho, self.name = be, ho, name
        scheme, N, bits = lp.CHAINS[name]
        self.bfv = scheme == "bfv"
        kw = dict(bit_sizes=list(bits), plain_bits=20 if self.bfv else 0, sec128=False)
        self.g = be.Context(be.SCHEME_BFV if self.bfv else be.SCHEME_CKKS, N, device=0, **kw)
        self.o = ho.Context(ho.SCHEME_BFV if self.bfv else ho.SCHEME_CKKS, N, **kw)
        assert self.g.moduli == self.o.moduli
        if name in lp.SHOUP_CHAINS:  # the Shoup build of the u64 engine: the chain's form and engines are the table's
            sr.check_device(name, self.g)
        self.N = N
        self.chain = lp.chain(scheme, N, bits, self.g.fp64)
        self.rng = np.random.default_rng(list(lp.CHAINS).index(name) + 77)
        self.rk = self.o.random_kswitch_key(self.rng)
        self.g.set_relin_key(self.rk)
        self.key_steps = tuple(rot_steps)
        self.gk = {}
        for s in rot_steps:
            e = self.o.galois_elt(s)
            self.gk[e] = self.o.random_kswitch_key(self.rng)
            self.g.set_galois_key(e, self.gk[e])
        self.g.set_latency_max(None)
        self.g.set_lds_max(None)
        self.host, self.dev, self.want, self.sent = {}, {}, {}, {}
        self.threads = max(1, min(8, ho.lib().ho_max_threads()))

    def close(self):
        self.g.close()

    def operands(self, L):
        """A, B [15, 2, L, N], C3 [15, 3, L, N] on the host and on the device"""
        if L not in self.host:
            o, rng, m = self.o, self.rng, N_TILE + N_TAIL
            A = np.stack([o.random_poly(rng, L, 2) for _ in range(m)])
            B = np.stack([o.random_poly(rng, L, 2) for _ in range(m)])
            A[-1] = eo.family(o, "qm1", L, 2, coeff_form=self.bfv)
            B[-1] = eo.family(o, "qm1", L, 2, coeff_form=self.bfv)
            if self.bfv:  # (a size-3 ciphertext in coefficient form; its last row every residue q - 1)
                C3 = np.stack([o.random_poly(rng, L, 3) for _ in range(m)])
                C3[-1] = eo.family(o, "qm1", L, 3, coeff_form=True)
            else:  # the tensor products: relinearize(C3[i]) is multiply_relin(A[i], B[i])
                C3 = np.stack([o.multiply_ntt(A[i], B[i]) for i in range(m)])
            self.host[L] = (A, B, C3)
            self.dev[L] = tuple(self.g.to_device(x) for x in (A, B, C3))
        return self.host[L], self.dev[L]

    def sentinel(self, n_u64):
        """a device slab of at least n_u64 sentinel words"""
        if n_u64 not in self.sent:
            self.sent[n_u64] = self.g.to_device(np.full(n_u64, SENT, dtype=np.uint64))
        return self.sent[n_u64]

    def expected(self, op, L):
        """[15, 2, L', N]: the oracle's result of op for each distinct pair"""
        base = {"multiply_relin_over_a": "multiply_relin", "multiply_relin_rescale_over_a": "multiply_relin_rescale"}.get(op, op)
        if not self.bfv and base in ("relinearize", "relinearize_rescale"):
            base = "multiply_" + base.replace("relinearize", "relin")
        key = (base, L)
        if key in self.want:
            return self.want[key]
        (A, B, C3), _ = self.operands(L)
        o, ho, m = self.o, self.ho, len(A)
        ar = np.arange(m)
        e1 = o.galois_elt(1)
        if base == "multiply_relin":
            w = o.batch_op(ho.OP_MUL_RELIN, A, ar, B, ar, self.rk, threads=self.threads)
        elif base == "multiply_relin_rescale":
            w = o.batch_op(ho.OP_MUL_RELIN_RESCALE, A, ar, B, ar, self.rk, threads=self.threads)
        elif base == "relinearize":
            w = np.stack([o.relinearize(C3[i], self.rk) for i in range(m)])
        elif base == "apply_galois":
            w = np.stack([o.apply_galois(A[i], e1, self.gk[e1]) for i in range(m)])
        elif base == "rotate_add_in_place":
            w = np.stack([o.add(B[i], g) for i, g in enumerate(self.expected("apply_galois", L))])
        elif base == "rotate_sum":
            w = []
            for i in range(m):
                t = A[i].copy()
                for s in lp.ROTATE_SUM_STEPS:
                    t = o.add(t, o.rotate(A[i], s, self.gk))
                w.append(t)
            w = np.stack(w)
        elif base == "rotate_each":
            w = np.stack([o.rotate(A[i], lp.EACH_STEPS[i % len(lp.EACH_STEPS)], self.gk) for i in range(m)])
        else:
            raise KeyError(op)
        self.want[key] = w
        return w


class States:
    """the chain states of the module, one device context alive at a time (the cases are ordered by chain)"""

    def __init__(self, be, ho):
        self.be, self.ho, self.cur = be, ho, None

    def get(self, name):
        if self.cur is None or self.cur.name != name:
            self.close()
            ops = {op for c, op, _, _ in lp.CASES if c == name}
            steps = lp.ROTATE_KEY_STEPS if ops & {"rotate_sum", "rotate_each"} else (1,)
            self.cur = ChainState(self.be, self.ho, name, steps)
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


def _copy(st, dst, dst_off, src, src_off, n_u64):
    rc = st.be.lib().he355_copy(st.g.h, C.c_void_p(dst.ptr.value + int(dst_off) * 8), C.c_void_p(src.ptr.value + int(src_off) * 8), int(n_u64) * 8)
    assert rc == 0, rc


def _rows(st, src, per, idx, guard=0):
    """a slab [guard words of sentinel | one row per entry of idx, row r = src[idx[r]] | guard words of sentinel]"""
    n = len(idx)
    buf = st.g.alloc(2 * guard + n * per)
    if guard:
        s = st.sentinel(guard)
        _copy(st, buf, 0, s, 0, guard)
        _copy(st, buf, guard + n * per, s, 0, guard)
    for r, i in enumerate(idx):
        _copy(st, buf, guard + r * per, src, int(i) * per, per)
    return buf


def _free(st, *bufs):
    for b in bufs:
        b.free()
        st.g._bufs.remove(b)


def _first_bad_row(got, want_rows, idx):
    for r in range(len(idx)):
        if not np.array_equal(got[r], want_rows[idx[r]]):
            bad = np.argwhere(got[r] != want_rows[idx[r]])
            return r, len(bad), bad[0].tolist()
    return None


def run_call(st, op, L, n, chunk=None, what=()):
    """one call of op over n rows: every row == the oracle's, the guards and the operands untouched; the path counters == the plan's"""
    g, be, N = st.g, st.be, st.N
    kind, rescale, apart = lp.OPS[op]
    (A, B, C3), (dA, dB, dC3) = st.operands(L)
    want = st.expected(op, L)
    idx = pair_of_rows(n)
    per2, per3, Lo = 2 * L * N, 3 * L * N, (L - 1 if rescale else L)
    out_per = 2 * Lo * N
    steps = [lp.EACH_STEPS[int(i) % len(lp.EACH_STEPS)] for i in idx] if op == "rotate_each" else None
    plan = lp.plan_call(st.chain, op, L, n, chunk or lp.DEFAULT_CHUNK, steps=steps, key_steps=st.key_steps)
    if PLAN_LOG:
        with open(PLAN_LOG, "a") as f:
            f.write(json.dumps(dict(chain=st.name, op=op, L=L, n=n, chunk=chunk, outcomes=sorted([d, str(v)] for d, v in lp.outcomes(st.chain, plan)),
                                    two_streams=any(c.stream for c in plan.chunks), launches=[list(l.key()) for l in plan.launches()])) + "\n")
    what = (st.name, op, f"L={L}", f"n={n}") + tuple(what)
    pw = be.Context.pairwise()
    bufs, checks = [], []  # checks: (slab, host rows, words per row, guard words) of operands that must come back unchanged
    over_a = kind == "product" and not apart
    if kind == "product":
        da = _rows(st, dA, per2, idx, guard=per2 if over_a else 0)
        db = _rows(st, dB, per2, idx)
        bufs += [da, db]
        checks.append((db, B, per2, 0))
        if not over_a:
            checks.append((da, A, per2, 0))
        a_view = View(da, per2 if over_a else 0, n * per2)
    elif kind == "size3":
        d3 = _rows(st, dC3, per3, idx)
        bufs.append(d3)
        checks.append((d3, C3, per3, 0))
    else:
        da = _rows(st, dA, per2, idx)
        bufs.append(da)
        checks.append((da, A, per2, 0))
    if over_a:
        slab, guard = da, per2
    elif op == "rotate_add_in_place":
        slab, guard = _rows(st, dB, per2, idx, guard=out_per), out_per
        bufs.append(slab)
    else:
        guard = out_per
        slab = g.alloc(2 * guard + n * out_per)
        bufs.append(slab)
        s = st.sentinel(out_per)
        for r in range(n + 2):
            _copy(st, slab, r * out_per, s, 0, out_per)
    out = View(slab, guard, n * out_per)
    g.sync()
    g.path_stats(reset=True)
    if kind == "product":
        g.multiply_relin(L, n, a_view, db, pw, out, rescale=rescale)
    elif op == "relinearize":
        g.relinearize(L, n, d3, out)
    elif op == "relinearize_rescale":
        g.relinearize_rescale(L, n, d3, out)
    elif op == "apply_galois":
        g.apply_galois(L, n, da, g.galois_elt(1), out)
    elif op == "rotate_add_in_place":
        g.rotate_add(L, n, da, 1, out, out)
    elif op == "rotate_sum":
        ks = g.rotate_sum(L, n, da, list(lp.ROTATE_SUM_STEPS), out)
    elif op == "rotate_each":
        g.rotate_each(L, n, da, steps, out)
    g.sync()
    stats = g.path_stats()
    try:
        flat = slab.download()
        assert (flat[:guard] == SENT).all(), what + ("the ciphertext of sentinel words BEFORE the output slab was written",
                                                     int(np.argmax(flat[:guard] != SENT)))
        tail = flat[len(flat) - guard:]
        assert (tail == SENT).all(), what + ("the ciphertext of sentinel words AFTER the output slab was written", int(np.argmax(tail != SENT)))
        got = flat[guard:guard + n * out_per].reshape(n, 2, Lo, N)
        bad = _first_bad_row(got, want, idx)
        assert bad is None, what + (f"row {bad[0]} of {n} (pair {idx[bad[0]]}) differs from the oracle in {bad[1]} words, first at [poly, prime, coefficient] = {bad[2]}",
                                    lp.describe(st.chain, plan))
        if over_a and rescale:  # what the smaller output left of operand a: its own words, unchanged
            rest = flat[guard + n * out_per:guard + n * per2]
            orig = np.concatenate([A[i].reshape(-1) for i in idx[(n * out_per) // per2:]])
            assert np.array_equal(rest, orig[len(orig) - len(rest):]), what + ("operand a beyond the output laid over it was changed",)
        for buf, host, per, gd in checks:
            rows = buf.download()[gd:gd + n * per].reshape((n,) + host.shape[1:])
            bad = _first_bad_row(rows, host, idx)
            assert bad is None, what + (f"an operand was changed: row {bad[0]}",)
        if op == "rotate_sum":
            assert ks == len(lp.rotation_trie_nodes(lp.ROTATE_SUM_STEPS, N, st.key_steps)) == plan.key_switches
        if DEFAULT_SHAPES:
            assert {k: stats[k] for k in lp.COUNTERS} == plan.counters(), what + (stats, lp.describe(st.chain, plan))
    finally:
        _free(st, *bufs)
    return stats


def test_pair_of_rows_layout():
    assert pair_of_rows(1).tolist() == [14] and pair_of_rows(3).tolist() == [12, 13, 14]
    assert pair_of_rows(8).tolist() == list(range(7, 15)) and pair_of_rows(10).tolist() == [0, 1] + list(range(7, 15))
    assert pair_of_rows(24).tolist() == [r % 7 for r in range(16)] + list(range(7, 15))


@pytest.mark.parametrize("dual", [True, False], ids=["two_streams", "one_stream"])
def test_mixed_shape_calls(be, oracle, dual):
    """body chunks in a throughput shape, the ragged last chunk in the LDS (`out` apart) or latency (`out` over operand a) shape"""
    name = "n8192_60_45_60_both_engines"
    st = ChainState(be, oracle, name, (1,))
    try:
        L = st.g.L
        st.g.set_dual_stream(dual)
        for op, chunk, n in lp.mixed_shape_calls(st.chain, L):
            st.g.set_chunk(chunk)
            stats = run_call(st, op, L, n, chunk, what=(f"chunk={chunk}", "two streams" if dual else "one stream"))
            if DEFAULT_SHAPES:
                small = stats["ks_lds"] + stats["ks_latency"]
                assert small == 1 and stats["ks_unfused"] + stats["ks_fused"] == 2, (op, chunk, n, stats)
    finally:
        st.close()


CASE_IDS = [f"{c}-{op}-L{lp.case_level(c, L)}" for c, op, L, _ in lp.CASES]


@pytest.mark.parametrize("direction", ["up", "down"])
@pytest.mark.parametrize("case", range(len(lp.CASES)), ids=CASE_IDS)
def test_selection_boundaries(states, case, direction):
    """the batch sizes boundary_cases derives for the case, ascending (each directly after a smaller one) or descending (after a larger)"""
    name, op, L, decisions = lp.CASES[case]
    st = states.get(name)
    L = lp.case_level(name, L)
    assert L <= st.g.L
    ns = lp.boundary_cases(st.chain, op, L, decisions)
    assert ns and ns[-1] <= lp.SCAN_MAX
    for n in (ns if direction == "up" else ns[::-1]):
        run_call(st, op, L, n, what=(direction,))
