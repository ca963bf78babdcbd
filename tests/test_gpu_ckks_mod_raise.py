"""he355_ckks_mod_raise and he355_ckks_lift_centred on the device, bit for bit against tests/ckks_mod_raise_ref.py (which
tests/test_ckks_mod_raise_ref_cpu.py holds to exact integers), the fused call also against the four-call composition on the device (copy row 0,
he355_ntt_inverse, he355_ckks_lift_centred, he355_ntt_forward), with sentinels around every output and the input re-read:

* rings: N = 1024 (the streaming route, asserted by he355_raise_stats), 2048, 4096 (LOGN1 = 1, 2) and 8192 on {60, 40, 40, 60}; at
  N = 32768 (LOGN1 = 5, the sources parked in LDS) one case with n = 2 on {60, 40, 40, 60} and one with n = 1 on {40, 60, 60} (an fp64 source, a u64 target);
* chains at N = 2048: {60, 40, 40, 60} (u64 source, fp64 targets), {40, 60, 60} (fp64 source, u64 target), {60, 60, 60}, {42, 38, 45, 44} (no u64
  prime, q_0 above a target), {60, 50, 40, 60} (the Shoup form), and from tests/explicit_moduli.py `tiny` (a 60-bit prime 0 over 14-bit moduli),
  `engine_edge_47`, and the primes of `ratio_two` with the 47-bit and the 46-bit one as prime 0 (he355_ctx_create_primes: q_0 right above and
  right below 2 q_1 -- the fixture's own order has the small prime first);
* operands: uniform, all 0, and the NTT images (the reference's forward transform) of the coefficient patterns of the core test: all q_0 - 1,
  both tie points, alternating, an impulse, the multiples of q_j and their neighbours;
* shapes: sizes 1, 2, 3; L_in = 1 and L_in = L_top with distinct garbage in rows >= 1; L_to = 1, 2, L_top; n on both sides of the chunk
  (he355_set_chunk(4): 3, 4, 5); n * size * 4 on both sides of the compute-unit count (torch's multi_processor_count restates the rule;
  split_launches is asserted and the two sides agree on the ciphertexts they share);
* hygiene: the sentinels stay, d_in is unchanged, the first call repeated after a larger and a smaller one gives the same bits, he355_raise_stats
  equals the plan, he355_path_stats / he355_hoist_stats / he355_poly_stats do not move;
* round trip: raise to L_top, he355_mod_switch_drop to 1, the input's row 0.
Every context is pinned to the chunk (1024) and the latency rule the restated plan assumes, so the module holds under HE355_CHUNK and
HE355_LATENCY_MAX too.
These tests fail on a library without the calls: the symbols do not exist."""
import functools
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ckks_mod_raise_ref as ref
import explicit_moduli as em
from bfv_gpu_helpers import At, be, inner_of, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

_RATIO = em.load()["ratio_two"]["primes"]
CHAINS = {
    "n1024_60_40_40_60": (1024, [60, 40, 40, 60]),
    "n2048_60_40_40_60": (2048, [60, 40, 40, 60]),
    "n4096_60_40_40_60": (4096, [60, 40, 40, 60]),
    "n8192_60_40_40_60": (8192, [60, 40, 40, 60]),
    "n2048_40_60_60": (2048, [40, 60, 60]),
    "n2048_60_60_60": (2048, [60, 60, 60]),
    "n2048_42_38_45_44": (2048, [42, 38, 45, 44]),
    "n2048_60_50_40_60_shoup": (2048, [60, 50, 40, 60]),
    "n2048_tiny": (2048, em.load()["tiny"]["primes"]),
    "n2048_engine_edge_47": (2048, em.load()["engine_edge_47"]["primes"]),
    "n2048_q0_above_2q1": (2048, [_RATIO[2], _RATIO[0], _RATIO[1], _RATIO[3]]),
    "n2048_q0_below_2q1": (2048, [_RATIO[1], _RATIO[0], _RATIO[2], _RATIO[3]]),
}


def contexts(be, oracle, N, chain):
    """the device context and the oracle's; the device context in the state plan() restates -- a chunk of 1024 ciphertexts and the library's own
    rule for the latency shapes -- whatever HE355_CHUNK / HE355_LATENCY_MAX say (tools/test_matrix.sh runs the suite under both)"""
    g, o = _contexts(be, oracle, N, chain)
    g.set_chunk(1024)
    g.set_latency_max(None)
    return g, o


def _contexts(be, oracle, N, chain):
    if max(chain) > 60:
        g = be.Context(be.SCHEME_CKKS, N, primes=list(chain), device=0)
        o = oracle.Context(oracle.SCHEME_CKKS, N, primes=list(chain))
    else:
        g = be.Context(be.SCHEME_CKKS, N, bit_sizes=chain, sec128=False, device=0)
        o = oracle.Context(oracle.SCHEME_CKKS, N, bit_sizes=chain, sec128=False)
    assert g.moduli == o.moduli
    return g, o


@functools.lru_cache(maxsize=None)
def cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process of its own, once per session: torch brings its own
    HIP runtime, which finds no device in a process where the library's has already opened it"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


class Pool:
    """the operands of one chain, each with its reference at L_top computed once: rows [P][N] (NTT form under q_0), coeff [P][N], want [P][L_top][N]"""

    def __init__(self, o, Lt, rng):
        q = [int(v) for v in o.moduli[:Lt]]
        pats = ref.patterns(q, o.N, rng)
        pats["uniform2"] = rng.integers(0, q[0], o.N, dtype=np.uint64)
        self.names = list(pats)
        self.coeff = np.stack([pats[k] for k in self.names])
        self.rows = np.stack([o.ntt(0, np.ascontiguousarray(c)) for c in self.coeff])
        self.rows[self.names.index("zero")] = 0
        self.want = np.stack([ref.mod_raise(o, r[None], Lt) for r in self.rows])
        self.next = 0

    def take(self, count):
        idx = [(self.next + k) % len(self.names) for k in range(count)]
        self.next = (self.next + count) % len(self.names)
        return idx


@pytest.fixture(scope="module", params=list(CHAINS))
def rctx(request, be, oracle):
    N, chain = CHAINS[request.param]
    g, o = contexts(be, oracle, N, chain)
    rng = np.random.default_rng(zlib.crc32(request.param.encode()))
    yield g, o, rng, Pool(o, g.L, rng), cu_count()
    g.close()


def make_input(o, rng, pool, idx, size, L_in):
    """[n][size][L_in][N]: row 0 of polynomial p is pool operand idx[p]; rows >= 1 distinct garbage (any 64-bit words: they are never read)"""
    polys = len(idx)
    x = rng.integers(0, 1 << 63, (polys, L_in, o.N), dtype=np.uint64) | np.uint64(1 << 63)
    x[:, 0] = pool.rows[idx]
    return x.reshape(polys // size, size, L_in, o.N)


def plan(g, cus, size, n, L_to, chunk=1024):
    """he355_raise_stats after one call, restated: chunks of min(chunk, n) ciphertexts, one launch each of the ring's route, split by the rule"""
    sizes = [min(chunk, n - off) for off in range(0, n, chunk)]
    work = L_to > 1
    fused = g.N > 1024
    return {"calls": 1, "chunks": len(sizes), "fused_launches": len(sizes) if work and fused else 0, "streaming_launches": len(sizes) if work and not fused else 0,
            "split_launches": sum(1 for nc in sizes if work and fused and ref.tsplit_rule(nc * size, L_to, cus) > 1)}


def run_raise(g, x, L_to, expect=None):
    n, size, L_in, N = x.shape
    d_in = g.to_device(x)
    d_out = sentinelled(g, n * size * L_to * N, N)
    g.raise_stats(reset=True)
    g.ckks_mod_raise(L_in, L_to, size, n, d_in, At(d_out, N))
    got = inner_of(d_out, N, "d_out").reshape(n * size, L_to, N)
    st = g.raise_stats()
    if expect is not None:
        assert st == expect, (st, expect)
    assert np.array_equal(d_in.download(x.shape), x), "d_in changed"
    d_in.free()
    d_out.free()
    return got


def run_composition(be, g, x, L_to):
    """the defining composition through public calls: copy row 0, he355_ntt_inverse, he355_ckks_lift_centred, he355_ntt_forward"""
    n, size, L_in, N = x.shape
    polys = n * size
    d_in, tmp, out = g.to_device(x), g.alloc(polys * N), g.alloc(polys * L_to * N)
    for p in range(polys):
        assert be.lib().he355_copy(g.h, At(tmp, p * N).ptr, At(d_in, p * L_in * N).ptr, N * 8) == be.OK
    g.ntt(tmp, polys, [0], inverse=True)
    g.ckks_lift_centred(L_to, polys, tmp, out)
    g.ntt(out, polys * L_to, list(range(L_to)))
    got = out.download((polys, L_to, N))
    for b in (d_in, tmp, out):
        b.free()
    return got


def shapes(Lt):
    """(size, n, L_in, L_to): every size, both input levels, L_to = 1, 2, L_top, one and several ciphertexts"""
    return [(1, 5, 1, Lt), (2, 3, Lt, Lt), (3, 2, 1, 2), (2, 4, Lt, 1), (3, 1, Lt, Lt), (2, 8, 1, Lt), (1, 1, 1, Lt), (2, 2, Lt, 2)]


def test_raise_against_the_reference_and_the_composition(rctx, be):
    g, o, rng, pool, cus = rctx
    Lt = g.L
    frozen = {k: f() for k, f in (("path", g.path_stats), ("hoist", g.hoist_stats), ("poly", g.poly_stats))}
    first = None
    for size, n, L_in, L_to in shapes(Lt):
        if L_to > Lt:
            continue
        idx = pool.take(n * size)
        x = make_input(o, rng, pool, idx, size, L_in)
        got = run_raise(g, x, L_to, plan(g, cus, size, n, L_to))
        for p, k in enumerate(idx):
            assert np.array_equal(got[p], pool.want[k][:L_to]), (size, n, L_in, L_to, "polynomial", p, pool.names[k])
        assert np.array_equal(got[:, 0], x.reshape(n * size, L_in, g.N)[:, 0]), "row 0 is the input's"
        assert np.array_equal(run_composition(be, g, x, L_to), got), (size, n, L_in, L_to, "the four-call composition")
        if first is None:
            first = (x, L_to, got)
    # the first call again, after larger and smaller ones
    assert np.array_equal(run_raise(g, first[0], first[1]), first[2])
    assert g.N > 1024 or g.raise_stats()["streaming_launches"] == 1
    assert {k: f() for k, f in (("path", g.path_stats), ("hoist", g.hoist_stats), ("poly", g.poly_stats))} == frozen


def test_the_input_level_and_its_garbage_do_not_matter(rctx):
    g, o, rng, pool, cus = rctx
    Lt = g.L
    idx = pool.take(4)
    a = make_input(o, rng, pool, idx, 2, 1)
    b = make_input(o, rng, pool, idx, 2, Lt)
    c = make_input(o, rng, pool, idx, 2, Lt)
    assert Lt == 1 or not np.array_equal(b[:, :, 1:], c[:, :, 1:])
    ga, gb, gc = (run_raise(g, x, Lt) for x in (a, b, c))
    assert np.array_equal(ga, gb) and np.array_equal(gb, gc)


def test_n_on_both_sides_of_the_chunk(rctx):
    g, o, rng, pool, cus = rctx
    Lt = g.L
    g.set_chunk(4)
    try:
        for n in (3, 4, 5):
            idx = pool.take(n * 2)
            got = run_raise(g, make_input(o, rng, pool, idx, 2, 1), Lt, plan(g, cus, 2, n, Lt, chunk=4))
            for p, k in enumerate(idx):
                assert np.array_equal(got[p], pool.want[k]), (n, "polynomial", p, pool.names[k])
    finally:
        g.set_chunk(1024)


def test_both_sides_of_the_compute_unit_count(rctx):
    g, o, rng, pool, cus = rctx
    Lt = g.L
    below, above = (cus - 1) // 4, -(-cus // 4)  # polynomials: the most with polys * 4 < CUs, the fewest with polys * 4 >= CUs
    assert below * 4 < cus <= above * 4
    idx = [k % len(pool.names) for k in range(above)]
    x = make_input(o, rng, pool, idx, 1, 1)
    pl_b, pl_a = plan(g, cus, 1, below, Lt), plan(g, cus, 1, above, Lt)
    if g.N > 1024 and Lt >= 3:
        assert pl_b["split_launches"] == 1 and pl_a["split_launches"] == 0
        assert ref.tsplit_rule(below, Lt, cus) == min(Lt - 1, -(-cus // (below * 4))) >= 2
    got_b, got_a = run_raise(g, x[:below], Lt, pl_b), run_raise(g, x, Lt, pl_a)
    assert np.array_equal(got_b, got_a[:below]), "the split and the unsplit launch differ"
    for p, k in enumerate(idx):
        assert np.array_equal(got_a[p], pool.want[k]), ("polynomial", p, pool.names[k])
    # one ciphertext: the split is as wide as the rule allows
    one = plan(g, cus, 2, 1, Lt)
    assert one["split_launches"] == (1 if g.N > 1024 and Lt >= 3 and 8 < cus else 0)
    got_1 = run_raise(g, x[:2].reshape(1, 2, 1, g.N), Lt, one)
    assert np.array_equal(got_1, got_a[:2])
    # the latency shapes switched off: no split, the same bits
    g.set_latency_max(0)
    try:
        off = dict(pl_b, split_launches=0)
        assert np.array_equal(run_raise(g, x[:below], Lt, off), got_b)
    finally:
        g.set_latency_max(None)


def test_lift_centred_on_its_own(rctx):
    g, o, rng, pool, cus = rctx
    Lt, N = g.L, g.N
    q = [int(v) for v in o.moduli[:Lt]]
    P = len(pool.names)
    d_in = g.to_device(pool.coeff)
    for L_to in sorted({1, min(2, Lt), Lt}):
        d_out = sentinelled(g, P * L_to * N, N)
        g.raise_stats(reset=True)
        g.ckks_lift_centred(L_to, P, d_in, At(d_out, N))
        got = inner_of(d_out, N, "d_out").reshape(P, L_to, N)
        assert g.raise_stats() == {"calls": 0, "chunks": 0, "fused_launches": 0, "streaming_launches": 1, "split_launches": 0}
        assert np.array_equal(got, ref.lift_centred(q, pool.coeff, L_to)), L_to
        assert np.array_equal(got[:, 0], pool.coeff)
        d_out.free()
    assert np.array_equal(d_in.download(pool.coeff.shape), pool.coeff)
    d_in.free()


def test_raise_then_drop_is_the_input(rctx):
    g, o, rng, pool, cus = rctx
    Lt, N = g.L, g.N
    idx = pool.take(6)
    x = make_input(o, rng, pool, idx, 2, 1)
    d_in, up, down = g.to_device(x), g.alloc(6 * Lt * N), g.alloc(6 * N)
    g.ckks_mod_raise(1, Lt, 2, 3, d_in, up)
    g.mod_switch_drop(Lt, 1, 6, up, down)
    assert np.array_equal(down.download(x.shape), x)
    for b in (d_in, up, down):
        b.free()


# LOGN1 = 5 is the one instantiation whose sources wait in LDS: a u64 source into fp64 targets (wide lift), and an fp64 source into a u64 target
@pytest.mark.parametrize("bits,names", [([60, 40, 40, 60], ["uniform", "alternating_ties", "multiples_of_q1", "all_q0_minus_1"]), ([40, 60, 60], ["uniform", "alternating_ties"])],
                         ids=["60_40_40_60_n2", "40_60_60_n1"])
def test_raise_at_n32768(be, oracle, bits, names):
    g, o = contexts(be, oracle, 32768, bits)
    rng = np.random.default_rng(32768 + len(bits))
    Lt, N, cus = g.L, g.N, cu_count()
    q = [int(v) for v in o.moduli[:Lt]]
    pats = ref.patterns(q, N, rng)
    rows = np.stack([o.ntt(0, np.ascontiguousarray(pats[k])) for k in names])
    x = rng.integers(0, 1 << 63, (len(names), Lt, N), dtype=np.uint64) | np.uint64(1 << 63)
    x[:, 0] = rows
    x = x.reshape(len(names) // 2, 2, Lt, N)
    got = run_raise(g, x, Lt, plan(g, cus, 2, len(names) // 2, Lt))
    for p, k in enumerate(names):
        assert np.array_equal(got[p], ref.mod_raise(o, rows[p][None], Lt)), k
    assert np.array_equal(run_composition(be, g, x, Lt), got)
    g.close()
