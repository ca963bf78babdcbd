"""The hoisted rotation family (csrc/he355_kernels_hoist.hip: he355_apply_galois_hoisted, he355_rotate_hoisted_plain_sum,
he355_rotate_hoisted_plain_sum_lazy, he355_linear_transform_bsgs, he355_plain_extend_special) held to its references -- tests/rotate_hoisted_ref.py,
rotate_hoisted_lazy_ref.py, linear_transform_bsgs_ref.py: Python integers over the oracle's transforms, themselves held on these chains by
tests/test_hoisted_layouts_ref_cpu.py -- on every layout of tests/hoisted_layouts.py, bit for bit (np.array_equal, no tolerance anywhere).
Run with -m gpu on an MI355X; nothing here skips.  The table says what each layout is for: the special prime in the fp64 engine
(hoist_sp_row<ArF64>, its `last` branch, logn1 = 2 and 5, under BFV), N = 16384 and 32768, the chains of tests/golden/explicit_moduli.json,
L = 1 and 2 under K = 5.

One device context per layout, shared by its cases (the cases are ordered by layout; one context is alive at a time), random keys for
steps 1, 3, -2; n = 2 ciphertexts, n = 1 at N >= 16384; levels L_top and L = 1 (deep_4096: L = 2 as well).  Every context asserts that the
device and the oracle hold the table's chain, that he355_prime_uses_fp64 follows explicit_moduli.is_f64 and the form explicit_moduli.form_of.

* eager: he355_apply_galois_hoisted over the elements 5, 5^(N/4) mod 2N, N + 1, N - 1, 3, 2N - 3, 2N - 1, 1 and 3 again, a random key
  installed for each keyed one (N >= 16384: 5^(N/4), 2N - 3, N - 1 and 1); BFV in both ntt_form values;
* sums: he355_rotate_hoisted_plain_sum and he355_rotate_hoisted_plain_sum_lazy over steps [0, 1, -2, 3, 1] and [3, 0];
* bsgs: he355_linear_transform_bsgs as baby [0, 1, -2] x giant [3, 0], [1, -2] x [3], and [0, 1] x [0, 3] under the mask [[1, 0], [1, 1]];
* extend: he355_plain_extend_special at the levels L >= 2 on coefficients uniform in (-q_0 / 2, q_0 / 2], with 0, 1, -1, floor(q_0 / 2),
  -floor(q_0 / 2) and -floor(q_0 / 2) + 1 planted in the first columns of the first plaintext, and the mismatch count of a plaintext with
  three planted disagreements;
* edges (hoisted_layouts.EDGED): ciphertexts, plaintexts (row L included) and the key of step 1 all q - 1, then c1 = 0, through the lazy
  sum and through the transform [0, 1] x [0, 1];
* every call: he355_hoist_stats by its rules (printed), he355_path_stats unchanged, sentinels on both sides of the output, the inputs
  re-read unchanged.

The run rule of k_bsgs_inner on the device (bsgs_run is the shortest run over the tiles of a launch: every tile folds at the 60-bit
prime's cut), one ciphertext, all operands and the key q - 1:
* two folds: N = 1024 {60,40,60} at L = 1 (both tiles 60-bit primes), 519 identity babies and one keyed one under giant [0]: 520 terms at
  run 256, folded after 256 terms and again after 511;
* folds under small moduli, 258 identity babies and one keyed one: tiny_n1024 at L = 4 (tiles of 60, 14, 16, 31 and 60 bits) and
  unsorted_small_special_n1024 at L = 3 (40, 50, 60 and 30 bits: the 60-bit prime is neither the first tile nor the last).
Not covered: a run of 337 or 1023 as the launch's run (every fixture chain that has such a prime also has a 256-term prime, and the launch
takes the shortest), and the cap of 2^16 terms (it needs 65537 terms).

A mismatch names layout, call, level, ciphertext, polynomial and prime.  profiles/hoisted_layouts.txt holds one run's output (-s)."""
import time
import zlib

import numpy as np
import pytest

import hoisted_layouts as hl
import linear_transform_bsgs_ref as bsgs
import rotate_hoisted_lazy_ref as lazy
import rotate_hoisted_ref as ref
from bfv_gpu_helpers import SENT, At, be, inner_of, pair, sentinelled  # noqa: F401 (be: the fixture)
from test_gpu_rotate_hoisted import make_bfv, make_ckks, rand_cts, random_keys

pytestmark = pytest.mark.gpu

T0 = time.time()
TIMES = {}
SUMS = ([0, 1, -2, 3, 1], [3, 0])
SPLITS = (([0, 1, -2], [3, 0], None), ([1, -2], [3], None), ([0, 1], [0, 3], [[1, 0], [1, 1]]))
RUN_RULE = {"tiny_n1024": 4, "unsorted_small_special_n1024": 3}  # layout: the level of its 259-term launch


def same(got, want, name, call, L):
    """bit for bit; the first difference by ciphertext, polynomial and prime"""
    assert got.shape == want.shape, (name, call, L, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    at = tuple(int(v) for v in bad[0])
    lead = at[:-4] if len(at) > 4 else ()
    pytest.fail(f"layout {name}, {call}, L = {L}: {len(bad)} words differ" + (f", block {lead}" if lead else "")
                + f", first at ciphertext {at[-4]}, polynomial {at[-3]}, prime {at[-2]}, position {at[-1]}: got {int(got[at])}, want {int(want[at])}")


class Calls:
    """a device context and the oracle's: operands at q - 1, the counters around a call, and the device calls -- each between sentinels,
    the inputs re-read unchanged"""

    def __init__(self, name, g, o):
        self.name, self.g, self.o, self.N = name, g, o, o.N

    def full_cts(self, L, n=1):
        o = self.o
        return np.stack([np.stack([np.stack([np.full(o.N, q - 1, dtype=np.uint64) for q in o.moduli[:L]])] * 2)] * n)

    def full_qp(self, L, count):
        o = self.o
        one = np.stack([np.full(o.N, q - 1, dtype=np.uint64) for q in o.moduli[:L] + [o.moduli[-1]]])
        return np.broadcast_to(one, (count, L + 1, o.N)).copy()

    def full_key(self):
        o = self.o
        top = np.empty((o.L, 2, o.K, o.N), dtype=np.uint64)
        for t, q in enumerate(o.moduli):
            top[:, :, t, :] = q - 1
        return top

    def counted(self, call, L, f, want):
        """f() between a reset of he355_hoist_stats and its reading: the counters of `want` hold, he355_path_stats does not move"""
        g = self.g
        g.hoist_stats(reset=True)
        paths = g.path_stats()
        out = f()
        st = g.hoist_stats()
        print(f"hoist {self.name} {call} L = {L}: " + ", ".join(f"{k} = {st[k]}" for k in ("digit_lifts", "key_products", "mod_downs", "inner_sums")))
        assert {k: st[k] for k in want} == want, (self.name, call, L, st, want)
        assert g.path_stats() == paths, (self.name, call, L, "he355_path_stats moved")
        return out

    def _call(self, call, L, words, inputs, launch):
        g, N = self.g, self.N
        bufs = [g.to_device(x) for x in inputs]
        d_out = sentinelled(g, words, N)
        launch(bufs, At(d_out, N))
        got = inner_of(d_out, N, (self.name, call, L))
        for k, (b, x) in enumerate(zip(bufs, inputs)):
            assert np.array_equal(b.download(x.shape), x), (self.name, call, L, "input", k, "was written")
            b.free()
        d_out.free()
        return got

    def eager(self, L, cts, elts, ntt_form):
        n = len(cts)
        got = self._call("apply_galois_hoisted", L, len(elts) * cts.size, [cts],
                         lambda b, out: self.g.apply_galois_hoisted(L, n, b[0], elts, out, ntt_form))
        return got.reshape((len(elts),) + cts.shape)

    def plain_sum(self, L, cts, steps, plains, is_lazy):
        n = len(cts)
        f = self.g.rotate_hoisted_plain_sum_lazy if is_lazy else self.g.rotate_hoisted_plain_sum
        call = "rotate_hoisted_plain_sum" + ("_lazy" if is_lazy else "")
        return self._call(call, L, cts.size, [cts, plains], lambda b, out: f(L, n, b[0], steps, b[1], out)).reshape(cts.shape)

    def transform(self, L, cts, baby, giant, plain_qp, mask=None):
        n = len(cts)
        return self._call("linear_transform_bsgs", L, cts.size, [cts, plain_qp],
                          lambda b, out: self.g.linear_transform_bsgs(L, n, b[0], baby, giant, b[1], out, mask)).reshape(cts.shape)


class Layout(Calls):
    """one layout's device and oracle contexts, its random keys {element: key} and its generator"""

    def __init__(self, be, oracle, name):
        e = hl.entry(name)
        self.e, self.bfv = e, e["scheme"] == "bfv"
        if not self.bfv:
            g, o = make_ckks(be, oracle, e["N"], e["bits"], primes=e["primes"])
        elif e["primes"] is None:
            g, o = make_bfv(be, oracle, e["N"], e["bits"], e["plain_bits"])
        else:
            g, o = pair(be, oracle, (e["N"], e["primes"], e["t"]))[:2]
        super().__init__(name, g, o)
        assert g.moduli == o.moduli and g.L == o.L == len(o.moduli) - 1 and g.t == o.t, (name, g.moduli, o.moduli)
        hl.check_chain(name, g.moduli)
        fp64, form = hl.engines(g.moduli)
        assert g.fp64 == fp64, (name, "the engines, by the prime itself", g.fp64)
        self.n = 1 if self.N >= 16384 else 2
        self.rng = np.random.default_rng(zlib.crc32(("layouts" + name).encode()))
        self.keys = random_keys(g, o, self.rng, steps=hl.STEPS, conj=False)
        bits = [int(q).bit_length() for q in g.moduli]
        print(f"\nlayout {name}: {e['scheme']} N = {self.N} bits {bits} t = {g.t} fp64 {[int(f) for f in fp64]} form {form} -- {e['for']}")

    def close(self):
        self.g.close()

    def levels(self):
        return hl.levels(self.name, self.g.L)

    def key_for(self, elt):
        """a random key for any odd element, installed once"""
        if elt != 1 and elt not in self.keys:
            self.keys[elt] = self.o.random_kswitch_key(self.rng)
            self.g.set_galois_key(elt, self.keys[elt])

    def rand_qp(self, L, count):
        return np.stack([self.o.random_poly(self.rng, L, 1, special=True)[0] for _ in range(count)])


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def case_eager(lay):
    o, N = lay.o, lay.N
    if N >= 16384:
        elts = [pow(5, N // 4, 2 * N), 2 * N - 3, N - 1, 1]
    else:
        elts = [5, pow(5, N // 4, 2 * N), N + 1, N - 1, 3, 2 * N - 3, 2 * N - 1, 1, 3]
    for e in elts:
        lay.key_for(e)
    keyed = sum(e != 1 for e in elts)
    for ntt_form in ((0, 1) if lay.bfv else (1,)):
        for L in lay.levels():
            cts = rand_cts(o, lay.rng, lay.n, L)
            call = f"apply_galois_hoisted (ntt_form {ntt_form})"
            got = lay.counted(call, L, lambda: lay.eager(L, cts, elts, ntt_form), {"digit_lifts": 1, "key_products": keyed, "mod_downs": keyed})
            want = ref.hoisted_many(o, cts, elts, lay.keys, ntt_form)
            for r, e in enumerate(elts):
                same(got[r], want[r], lay.name, f"{call}, element {e} (block {r})", L)


def case_sums(lay):
    o = lay.o
    for L in lay.levels():
        cts = rand_cts(o, lay.rng, lay.n, L)
        plain_qp = lay.rand_qp(L, len(SUMS[0]))
        for steps in SUMS:
            keyed = sum(s != 0 for s in steps)
            pq = np.ascontiguousarray(plain_qp[:len(steps)])
            got = lay.counted(f"plain_sum_lazy {steps}", L, lambda: lay.plain_sum(L, cts, steps, pq, True),
                              {"digit_lifts": 1, "key_products": keyed, "mod_downs": 1})
            same(got, lazy.plain_sum_lazy(o, cts, steps, lay.keys, pq), lay.name, f"rotate_hoisted_plain_sum_lazy {steps}", L)
            pt = np.ascontiguousarray(pq[:, :L])
            got = lay.counted(f"plain_sum {steps}", L, lambda: lay.plain_sum(L, cts, steps, pt, False),
                              {"digit_lifts": 1, "key_products": keyed, "mod_downs": keyed})
            same(got, ref.plain_sum(o, cts, steps, lay.keys, pt), lay.name, f"rotate_hoisted_plain_sum {steps}", L)


def bsgs_counters(o, baby, giant, mask):
    """he355_hoist_stats of one chunk: one lift for the keyed babies and one per used keyed giant row; a key product per used keyed baby and
    per used keyed row; that row's mod-down and the last one; an inner sum per used row"""
    m = bsgs.used(mask, len(giant), len(baby))
    kb = sum(1 for i, s in enumerate(baby) if s and m[:, i].any())
    kg = sum(1 for j, s in enumerate(giant) if s and m[j].any())
    return {"digit_lifts": (kb > 0) + kg, "key_products": kb + kg, "mod_downs": kg + 1, "inner_sums": int(sum(m[j].any() for j in range(len(giant))))}


def case_bsgs(lay):
    o = lay.o
    for L in lay.levels():
        cts = rand_cts(o, lay.rng, lay.n, L)
        for baby, giant, mask in SPLITS:
            plain_qp = lay.rand_qp(L, len(giant) * len(baby)).reshape(len(giant), len(baby), L + 1, o.N)
            call = f"linear_transform_bsgs {baby} x {giant}" + (f" mask {mask}" if mask else "")
            got = lay.counted(call, L, lambda: lay.transform(L, cts, baby, giant, plain_qp, mask), bsgs_counters(o, baby, giant, mask))
            same(got, bsgs.linear_transform_bsgs(o, cts, baby, giant, lay.keys, plain_qp, mask), lay.name, call, L)


def centred_plain(o, c, L):
    """[L][N] NTT form of the integer coefficients c"""
    return np.stack([o.ntt(i, np.asarray(c % q, dtype=object).astype(np.uint64)) for i, q in enumerate(o.moduli[:L])])


def case_extend(lay):
    g, o, N = lay.g, lay.o, lay.N
    q0 = o.moduli[0]
    h = q0 // 2
    for L in [L for L in lay.levels() if L >= 2]:
        draws = [(lay.rng.integers(0, q0, N, dtype=np.uint64).astype(object) - h) for _ in range(3)]  # q_0 odd: [-h, h] = (-q_0 / 2, q_0 / 2]
        draws[0][:6] = [0, 1, -1, h, -h, -h + 1]
        plains = np.stack([centred_plain(o, c, L) for c in draws])
        # three planted disagreements in the last plaintext: coefficient k under prime i >= 1 is c + 1
        spots = [(3, 1), (N // 2, L - 1), (N - 1, 1)]
        for i in sorted({i for _, i in spots}):
            coeff = o.intt(i, plains[2, i])
            for k in [k for k, pi in spots if pi == i]:
                coeff[k] = (int(coeff[k]) + 1) % o.moduli[i]
            plains[2, i] = o.ntt(i, coeff)
        want = [lazy.extend_special(o, p) for p in plains]
        assert [w[1] for w in want] == [0, 0, 3], (lay.name, L, "the reference counts the planted disagreements")
        for count, wbad in ((2, 0), (3, 3)):
            src = np.ascontiguousarray(plains[:count])
            d_bad = g.to_device(np.full(1, SENT, dtype=np.uint64))
            got = lay._call("plain_extend_special", L, count * (L + 1) * N, [src],
                            lambda b, out: g.plain_extend_special(L, count, b[0], out, d_bad)).reshape(count, 1, L + 1, N)
            bad = int(d_bad.download()[0])
            d_bad.free()
            same(got, np.stack([w[0] for w in want[:count]])[:, None], lay.name, "plain_extend_special (ciphertext: the plaintext)", L)
            assert bad == wbad, (lay.name, "plain_extend_special mismatch count", L, bad, wbad)
        got = lay._call("plain_extend_special", L, 2 * (L + 1) * N, [np.ascontiguousarray(plains[:2])],
                        lambda b, out: g.plain_extend_special(L, 2, b[0], out)).reshape(2, 1, L + 1, N)
        same(got, np.stack([w[0] for w in want[:2]])[:, None], lay.name, "plain_extend_special without the check", L)


def case_edges(lay):
    g, o = lay.g, lay.o
    L = g.L
    e1 = o.galois_elt(1)
    top = lay.full_key()
    g.set_galois_key(e1, top)
    keys = {e1: top}
    try:
        cts = lay.full_cts(L)
        steps = [0, 1, 1]
        same(lay.plain_sum(L, cts, steps, lay.full_qp(L, 3), True), lazy.plain_sum_lazy(o, cts, steps, keys, lay.full_qp(L, 3)),
             lay.name, "rotate_hoisted_plain_sum_lazy, all q - 1", L)
        pq = lay.full_qp(L, 4).reshape(2, 2, L + 1, o.N)
        same(lay.transform(L, cts, [0, 1], [0, 1], pq), bsgs.linear_transform_bsgs(o, cts, [0, 1], [0, 1], keys, pq),
             lay.name, "linear_transform_bsgs [0, 1] x [0, 1], all q - 1", L)
        # c1 = 0: the baby key products are zero whatever the key
        z = rand_cts(o, lay.rng, 1, L)
        z[:, 1] = 0
        pr = lay.rand_qp(L, 4)
        got = lay.plain_sum(L, z, steps, pr[:3].copy(), True)
        same(got, lazy.plain_sum_lazy(o, z, steps, keys, pr[:3]), lay.name, "rotate_hoisted_plain_sum_lazy, c1 = 0", L)
        assert not got[0, 1].any(), (lay.name, "c1 = 0: polynomial 1 of the lazy sum is zero")
        pq = pr.reshape(2, 2, L + 1, o.N)
        same(lay.transform(L, z, [0, 1], [0, 1], pq), bsgs.linear_transform_bsgs(o, z, [0, 1], [0, 1], keys, pq),
             lay.name, "linear_transform_bsgs [0, 1] x [0, 1], c1 = 0", L)
    finally:
        g.set_galois_key(e1, lay.keys[e1])


def run_rule(g, o, name, L, n_ident, keys, transform):
    """n_ident identity babies and one keyed one under giant [0]; one ciphertext, every operand q - 1"""
    baby = [0] * n_ident + [1]
    one = np.stack([np.full(o.N, q - 1, dtype=np.uint64) for q in o.moduli[:L] + [o.moduli[-1]]])
    cts = np.stack([np.stack([one[:L]] * 2)])
    plain_qp = np.broadcast_to(one, (1, len(baby), L + 1, o.N)).copy()
    runs = [min(1 << 16, ((1 << 128) - 1) // ((q - 1) ** 2)) for q in o.moduli[:L] + [o.moduli[-1]]]
    print(f"hoist {name} run rule L = {L}: {len(baby)} terms, runs of the tiles {runs}, the launch's {min(runs)}")
    assert min(runs) == 256, (name, runs)
    call = f"linear_transform_bsgs, {n_ident} identity babies and one keyed"
    same(transform(L, cts, baby, [0], plain_qp), bsgs.linear_transform_bsgs(o, cts, baby, [0], keys, plain_qp), name, call, L)


def case_run_rule(lay):
    g, o = lay.g, lay.o
    L = RUN_RULE[lay.name]
    assert L == g.L
    e1 = o.galois_elt(1)
    top = lay.full_key()
    g.set_galois_key(e1, top)
    try:
        lay.counted("run rule", L, lambda: run_rule(g, o, lay.name, L, 258, {e1: top}, lay.transform),
                    {"digit_lifts": 1, "key_products": 1, "mod_downs": 1, "inner_sums": 1})
    finally:
        g.set_galois_key(e1, lay.keys[e1])


CASE = {"eager": case_eager, "sums": case_sums, "bsgs": case_bsgs, "extend": case_extend, "edges": case_edges, "run_rule": case_run_rule}


def cases():
    out = []
    for name in hl.LAYOUTS:
        out += [(name, c) for c in ("eager", "sums", "bsgs", "extend")]
        if name in hl.EDGED:
            out.append((name, "edges"))
        if name in RUN_RULE:
            out.append((name, "run_rule"))
    return out


class Layouts:
    """one device context alive at a time (the cases are ordered by layout)"""

    def __init__(self, be, oracle):
        self.be, self.oracle, self.cur = be, oracle, None

    def get(self, name):
        if self.cur is None or self.cur.name != name:
            self.close()
            self.cur = Layout(self.be, self.oracle, name)
        return self.cur

    def close(self):
        if self.cur is not None:
            self.cur.close()
            self.cur = None


@pytest.fixture(scope="module")
def layouts(be, oracle):
    s = Layouts(be, oracle)
    yield s
    s.close()
    if TIMES:
        worst = max(TIMES, key=TIMES.get)
        print(f"\nhoist wall time of the module: {time.time() - T0:.1f} s over {len(TIMES)} tests; the slowest: {worst} {TIMES[worst]:.2f} s")


@pytest.mark.parametrize("name,case", cases(), ids=["-".join(c) for c in cases()])
def test_layout(layouts, name, case):
    t = time.time()
    CASE[case](layouts.get(name))
    TIMES[f"{name}-{case}"] = time.time() - t


def test_run_rule_two_folds(be, oracle):
    """520 terms at run 256 under two 60-bit tiles: the sums fold after 256 terms and again after 511"""
    t = time.time()
    g, o = make_ckks(be, oracle, 1024, [60, 40, 60])
    lay = Calls("n1024_60_40_60", g, o)
    e1 = o.galois_elt(1)
    top = lay.full_key()
    g.set_galois_key(e1, top)
    assert [int(q).bit_length() for q in o.moduli] == [60, 40, 60]
    try:
        lay.counted("run rule, two folds", 1, lambda: run_rule(g, o, lay.name, 1, 519, {e1: top}, lay.transform),
                    {"digit_lifts": 1, "key_products": 1, "mod_downs": 1, "inner_sums": 1})
    finally:
        g.close()
    TIMES["run_rule_two_folds"] = time.time() - t
