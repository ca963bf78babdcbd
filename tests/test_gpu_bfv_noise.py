"""GPU parity of he355_bfv_noise_budget (Decryptor::invariant_noise_budget, batched) with the reference model in Python integers
(tests/bfv_noise_model.py: the phase from the oracle, then times t, CRT, centred magnitude, bit length) -- exact equality of d_budget and
d_noise_bits, no tolerance:

* uniform random ciphertexts, sizes 2 and 3, every level, n = 1, 5 and a batch the implementation cuts (budget 0, noise_bits exact);
* engineered ciphertexts (c1 = 0) whose phase composes to the edge values of the centring and bit-length code, one per ciphertext;
* real ciphertexts through the device pipeline (encrypt, multiply, relinearize, rotate, mod_switch to every level, plaintext operands),
  with the semantic statement: where the budget is positive, he355_decrypt + he355_bfv_decode return the expected slots;
* a ciphertext squared until its budget is 0;
* ordering behind an asynchronous producer, d_noise_bits = NULL, n = 0, every argument error, no raw hipMalloc in a second call."""
import ctypes as C

import numpy as np
import pytest

import bfv_gpu_helpers as helpers
import bfv_noise_model as model
from bfv_gpu_helpers import be, refused  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu


def chunk_of(N):
    """ciphertexts the implementation takes per chunk (DeviceContext::noise_chunk: 2^21 coefficients' worth, 64 to 1024, and never more
    than he355_set_chunk allows): a batch above it is cut"""
    return min(1024, max(64, (1 << 21) // N))


ALL = dict(helpers.ALL)
# 16 data primes, both engines, any order (the first chain of 17 in tests/test_bfv_level_core_cpu.py)
ALL["n1024_16primes"] = (1024, [60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 60, 40, 45, 50, 55, 59, 60], 20)


def want_of(o, cts, sk):
    """model (budget [n], noise_bits [n]) of host ciphertexts [n][size][L][N]"""
    w = [model.noise_of(o, ct, sk) for ct in cts]
    return np.array([b for _, b, _ in w], dtype=np.int32), np.array([nb for nb, _, _ in w], dtype=np.int32)


def check(g, o, sk, L, size, dbuf, host, tag):
    """device budget / noise_bits of the slab dbuf == model of its host copy; returns the model's (budget, noise_bits)"""
    n = len(host)
    budget, bits = g.bfv_noise_budget(L, size, n, dbuf, with_bits=True)
    wb, wn = want_of(o, host, sk)
    print(tag, "L", L, "size", size, "noise_bits", bits.tolist(), "want", wn.tolist(), "budget", budget.tolist(), "want", wb.tolist())
    assert budget.dtype == np.int32 and bits.dtype == np.int32
    assert np.array_equal(bits, wn), (tag, L, size, bits, wn)
    assert np.array_equal(budget, wb), (tag, L, size, budget, wb)
    return wb, wn


@pytest.mark.parametrize("name", list(ALL))
def test_uniform_random_ciphertexts(be, oracle, name):
    """a uniform phase: every word of the composition is exercised, the budget is 0"""
    g, o, N, sk, _ = helpers.pair(be, oracle, ALL[name], keys=True)
    rng = np.random.default_rng(31)
    big = chunk_of(N) + 6
    for L in range(1, g.L + 1):
        for size in (2, 3):
            base = np.stack([o.random_poly(rng, L, size) for _ in range(7)])
            wb, wn = want_of(o, base, sk)
            assert not wb.any(), (name, L, size, wb, "a uniform phase has no budget left")
            # n = 1 and 5 in one chunk; 70 cut in chunks of 3 (he355_set_chunk); and, at the top level and at L = 1, a batch above the
            # chunk the library takes by itself
            cases = [(1, None), (5, None), (70, 3)]
            if (L, size) in ((g.L, 3), (1, 2)):
                cases.append((big, None))
            for n, chunk in cases:
                idx = np.arange(n)
                if n > 7:
                    idx = (idx * 3 + 1) % 7  # neighbours differ, so every cut falls between unequal ciphertexts
                src = g.to_device(base[idx])
                g.set_chunk(chunk or 1024)
                budget, bits = g.bfv_noise_budget(L, size, n, src, with_bits=True)
                g.set_chunk(1024)
                assert np.array_equal(bits, wn[idx]), (name, L, size, n, chunk, bits, wn[idx])
                assert np.array_equal(budget, wb[idx]), (name, L, size, n, chunk)
                src.free()
    g.close()


@pytest.mark.parametrize("name", list(ALL))
def test_engineered_edge_values(be, oracle, name):
    """c1 = 0, so the phase is c0: one coefficient of c0 holds the residues of x t^-1 mod q_L for an edge value x, the rest are zero; one
    edge per ciphertext, so neighbours of a batch have norms from 0 bits to bits(q_L) - 1 and a leak across ciphertexts would show"""
    g, o, N, sk, _ = helpers.pair(be, oracle, ALL[name], keys=True)
    t = o.t
    for L in range(1, g.L + 1):
        qs = o.moduli[:L]
        qL = model.q_product(qs)
        vals = model.edge_values(qL)
        n = len(vals)
        cts = np.zeros((n, 2, L, N), dtype=np.uint64)
        for r, x in enumerate(vals):
            pos = (0, N - 1, N // 2, 255, 256)[r % 5] if r < 10 else (r * 37 + 5) % N
            cts[r, 0, :, pos] = model.residues_for(x, qs, t)
        want_bits = np.array([model.magnitude_bits(x, qL) for x in vals], dtype=np.int32)
        want_budget = np.maximum(0, qL.bit_length() - want_bits - 1).astype(np.int32)
        d = g.to_device(cts)
        budget, bits = g.bfv_noise_budget(L, 2, n, d, with_bits=True)
        assert np.array_equal(bits, want_bits), (name, L, bits, want_bits)
        assert np.array_equal(budget, want_budget), (name, L, budget, want_budget)
        wb, wn = want_of(o, cts[:8], sk)  # and the same through the oracle's phase, for the first ones
        assert np.array_equal(wn, want_bits[:8]) and np.array_equal(wb, want_budget[:8])
        d.free()
    g.close()


def centred(v, t):
    v = np.asarray(v).astype(object) % t
    return np.where(v > t // 2, v - t, v).astype(np.int64)


def slots_of(g, L, size, n, dbuf, N):
    dec, vals = g.alloc(n * N), g.alloc(n * N)
    g.decrypt(L, size, n, dbuf, dec)
    g.bfv_decode(n, dec, vals)
    out = vals.download().view(np.int64).reshape(n, N)
    dec.free()
    vals.free()
    return out


@pytest.mark.parametrize("name", ["n1024", "n4096_d3", "n8192_default", "n1024_16primes"])
def test_device_pipeline_real_keys(be, oracle, name):
    g, o, N, sk, pk = helpers.pair(be, oracle, ALL[name], keys=True)
    t, L = o.t, g.L
    codec = oracle.BatchCodec(N, t)
    rng = np.random.default_rng(41)
    rk = o.keygen_relin(sk, 23)
    elt = o.galois_elt(1)
    gk = o.keygen_galois(sk, elt, 24)
    g.set_relin_key(rk)
    g.set_galois_key(elt, gk)
    n = 3
    x, y, p, r = (rng.integers(-(t // 2), t // 2 + 1, (n, N)) for _ in range(4))
    enc = lambda v: np.stack([codec.encode(row) for row in v])
    cx, cy = g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
    g.encrypt(n, g.to_device(enc(x)), 31, 0, cx)
    g.encrypt(n, g.to_device(enc(y)), 31, n, cy)

    def stage(tag, dbuf, size, Ls, slots):
        """budget == model; where it is positive, the device decrypts to `slots`"""
        host = dbuf.download((n, size, Ls, N))
        wb, _ = check(g, o, sk, Ls, size, dbuf, host, f"{name} {tag}")
        got = slots_of(g, Ls, size, n, dbuf, N)
        for k in range(n):
            if wb[k] > 0:
                assert np.array_equal(got[k], slots[k]), (name, tag, Ls, k, "positive budget, wrong slots")
        return wb

    b_fresh = stage("fresh", cx, 2, L, centred(x, t))
    assert (b_fresh > 0).all()
    c3 = g.alloc(n * 3 * L * N)
    g.bfv_multiply(L, n, cx, cy, be.Context.pairwise(), c3)
    xy = centred(x.astype(object) * y.astype(object), t)
    b_mul = stage("multiply", c3, 3, L, xy)
    assert (b_mul < b_fresh).all()
    c2 = g.alloc(n * 2 * L * N)
    g.relinearize(L, n, c3, c2)
    stage("relinearize", c2, 2, L, xy)
    rot = g.alloc(n * 2 * L * N)
    g.rotate(L, n, c2, 1, rot)
    half = N // 2
    xy_rot = np.concatenate([np.roll(xy[:, :half], -1, axis=1), np.roll(xy[:, half:], -1, axis=1)], axis=1)
    stage("rotate", rot, 2, L, xy_rot)
    for L_to in range(L, 0, -1):
        low = g.alloc(n * 2 * L_to * N)
        g.bfv_mod_switch(L, L_to, 2, n, c2, low)
        stage(f"switch{L_to}", low, 2, L_to, xy)
        low3 = g.alloc(n * 3 * L_to * N)
        g.bfv_mod_switch(L, L_to, 3, n, c3, low3)
        stage(f"switch{L_to}_size3", low3, 3, L_to, xy)
        low.free()
        low3.free()
    mp, ap = g.alloc(n * 2 * L * N), g.alloc(n * 2 * L * N)
    g.bfv_multiply_plain(L, 2, n, cx, g.to_device(enc(p)), be.Context.pairwise(), mp)
    stage("multiply_plain", mp, 2, L, centred(x.astype(object) * p.astype(object), t))
    g.bfv_add_plain(L, 2, n, mp, g.to_device(enc(r)), be.Context.pairwise(), ap)
    stage("add_plain", ap, 2, L, centred(x.astype(object) * p.astype(object) + r.astype(object), t))
    g.close()


@pytest.mark.parametrize("name", ["n4096_d3", "n1024"])
def test_squared_until_no_budget(be, oracle, name):
    g, o, N, sk, pk = helpers.pair(be, oracle, ALL[name], keys=True)
    t, L = o.t, g.L
    codec = oracle.BatchCodec(N, t)
    rng = np.random.default_rng(43)
    g.set_relin_key(o.keygen_relin(sk, 23))
    n = 2
    x = rng.integers(-(t // 2), t // 2 + 1, (n, N))
    ct, c3 = g.alloc(n * 2 * L * N), g.alloc(n * 3 * L * N)
    g.encrypt(n, g.to_device(np.stack([codec.encode(row) for row in x])), 33, 0, ct)
    history = []
    for step in range(8):
        wb, wn = check(g, o, sk, L, 2, ct, ct.download((n, 2, L, N)), f"{name} squared x{step}")
        history.append(int(wb.max()))
        if not wb.any():
            break
        g.bfv_multiply(L, n, ct, ct, be.Context.pairwise(), c3)
        g.relinearize(L, n, c3, ct)
    assert history[0] > 0 and history[-1] == 0, history
    assert all(a >= b for a, b in zip(history, history[1:])), history
    g.close()


@pytest.mark.parametrize("name", ["n8192_default", "n1024"])
def test_budget_right_behind_an_asynchronous_multiply(be, oracle, name):
    """he355_bfv_multiply returns with its kernels queued (the batch cut in chunks of 3 over both streams); the budget is asked at once"""
    g, o, N, sk, pk = helpers.pair(be, oracle, ALL[name], keys=True)
    t, L, n = o.t, g.L, 8
    codec = oracle.BatchCodec(N, t)
    rng = np.random.default_rng(44)
    g.set_dual_stream(True)
    g.set_chunk(3)
    x = rng.integers(-(t // 2), t // 2 + 1, (2 * n, N))
    cts = g.alloc(2 * n * 2 * L * N)
    g.encrypt(2 * n, g.to_device(np.stack([codec.encode(row) for row in x])), 35, 0, cts)
    host = cts.download((2 * n, 2, L, N))
    prod = np.stack([o.bfv_multiply(host[k], host[n + k]) for k in range(n)])
    wb, wn = want_of(o, prod, sk)
    for rep in range(3):
        c3 = g.to_device(np.zeros(n * 3 * L * N, dtype=np.uint64))
        g.sync()
        g.bfv_multiply(L, n, cts, cts, be.Context.pairwise(0, n), c3)
        budget, bits = g.bfv_noise_budget(L, 3, n, c3, with_bits=True)
        assert np.array_equal(bits, wn) and np.array_equal(budget, wb), (name, rep, bits, wn)
        assert np.array_equal(c3.download((n, 3, L, N)), prod)
        c3.free()
    g.close()


def test_arguments(be, oracle):
    g, o, N, sk, pk = helpers.pair(be, oracle, "n4096_d3")
    L, n = g.L, 3
    rng = np.random.default_rng(45)
    cts = np.stack([o.random_poly(rng, L, 2) for _ in range(n)])
    d = g.to_device(cts)
    lib = be.lib()
    SENT = np.uint64(0x5E17155E17155E17)
    out = g.to_device(np.full(2 * n, SENT, dtype=np.uint64))
    raw = lambda L_, size, n_, ct, bud, nb: lib.he355_bfv_noise_budget(g.h, L_, size, n_, ct, bud, nb)
    bits_ptr = C.c_void_p(out.ptr.value + 4 * n)
    # no secret key yet
    assert raw(L, 2, n, d.ptr, out.ptr, bits_ptr) == be.E_INVALID_ARGS and b"secret key" in lib.he355_last_error()
    refused(be, lambda: g.bfv_noise_budget(L, 2, n, d))
    sk = o.keygen_secret(21)
    g.set_secret_key(sk)
    for bad in ((L, 1), (L, 4), (0, 2), (L + 1, 2), (-1, 2)):
        refused(be, lambda: g.bfv_noise_budget(bad[0], bad[1], n, d))
        assert raw(bad[0], bad[1], n, d.ptr, out.ptr, bits_ptr) == be.E_INVALID_ARGS and lib.he355_last_error()
    assert raw(L, 2, n, None, out.ptr, bits_ptr) == be.E_INVALID_ARGS and lib.he355_last_error()
    assert raw(L, 2, n, d.ptr, None, bits_ptr) == be.E_INVALID_ARGS and lib.he355_last_error()
    # n = 0: OK, nothing touched (null pointers included)
    assert raw(L, 2, 0, d.ptr, out.ptr, bits_ptr) == be.OK
    assert raw(L, 2, 0, None, None, None) == be.OK
    g.sync()
    assert (out.download() == SENT).all(), "a refused call and n = 0 leave the outputs as they were"
    assert len(g.bfv_noise_budget(L, 2, 0, d)) == 0
    # d_noise_bits = NULL: the budget alone, the word behind it untouched
    wb, wn = want_of(o, cts, sk)
    assert raw(L, 2, n, d.ptr, out.ptr, None) == be.OK
    got = out.download()
    assert np.array_equal(got.view(np.int32)[:n], wb)
    assert (got[(n * 4 + 7) // 8:] == SENT).all()
    assert np.array_equal(g.bfv_noise_budget(L, 2, n, d), wb)
    # with the bits
    assert raw(L, 2, n, d.ptr, out.ptr, bits_ptr) == be.OK
    got = out.download().view(np.int32)
    assert np.array_equal(got[:n], wb) and np.array_equal(got[n:2 * n], wn)
    g.close()
    # a CKKS context with a device is refused as one without
    gc = be.Context(be.SCHEME_CKKS, 4096, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    dc = gc.alloc(2 * gc.L * 4096)
    refused(be, lambda: gc.bfv_noise_budget(gc.L, 2, 1, dc))
    gc.close()


def test_second_call_makes_no_raw_allocation(be, oracle):
    g, o, N, sk, pk = helpers.pair(be, oracle, "n8192_default", keys=True)
    rng = np.random.default_rng(46)
    L, n = g.L, chunk_of(N) + 6
    base = np.stack([o.random_poly(rng, L, 3) for _ in range(4)])
    d = g.to_device(base[np.arange(n) % 4])
    out = g.alloc(n)
    bits_ptr = C.c_void_p(out.ptr.value + 4 * n)
    stats, res = [], []
    for _ in range(3):
        assert be.lib().he355_bfv_noise_budget(g.h, L, 3, n, d.ptr, out.ptr, bits_ptr) == be.OK
        g.sync()
        stats.append(g.alloc_stats())
        res.append(out.download())
    assert stats[0]["raw_mallocs"] == stats[1]["raw_mallocs"] == stats[2]["raw_mallocs"], stats
    assert stats[0]["raw_frees"] == stats[1]["raw_frees"] == stats[2]["raw_frees"], stats
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[1], res[2])
    wb, wn = want_of(o, base, sk)
    assert np.array_equal(res[0].view(np.int32)[:n], wb[np.arange(n) % 4]) and np.array_equal(res[0].view(np.int32)[n:], wn[np.arange(n) % 4])
    g.close()
