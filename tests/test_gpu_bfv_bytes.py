"""GPU parity of the PIR database codec (he355_bfv_bytes_per_plain, he355_bfv_unpack_bytes, he355_bfv_unpack_bytes_ntt, he355_bfv_pack_bytes),
bit-exact (np.array_equal, no tolerance):

* chains: n1024 (the routed path, Shoup form), (2048, {60, 40, 60}, 20) (the smallest column pass, both engines), n4096_d3 (fold form),
  (2048, {60, 40, 60}, 17) (w = 16: fields never straddle a byte) and (2048, {60, 40, 60}, 22) (w = 21);
* unpack / pack against numpy bit arithmetic (bfv_bytes_ref.np_fields, held to int.from_bytes in test_bfv_bytes_core_cpu.py): n in {1, 3}; B in {1, 9, Bmax - 1, Bmax}; strides B
  (contiguous: every plaintext but the first starts unaligned when B is odd), B + 5 and 8 ceil(B / 8) + 8; the slab starts 3 bytes into the
  buffer; 0xFF filler before, between and after the plaintexts; a sentinel plaintext before and after the output; the input read back
  unchanged.  pack (strides 8 ceil(B / 8) and 8 ceil(B / 8) + 8, clean coefficients and ones with junk above bit w) gives the bytes back,
  zeroes the tail of its last word and leaves the filler inside the stride, and the words before and after the slab, untouched;
* he355_bfv_unpack_bytes_ntt == he355_bfv_unpack_bytes + he355_bfv_plain_to_ntt: the same chains, L_out in {1, L_top}, n in {1, 3},
  B in {9, Bmax}, contiguous from byte 3; once more directly behind an unsynchronised he355_copy that produces the byte slab;
* refusals: a CKKS context, L_out outside 1..L_top, B == 0, B > Bmax, stride < B, (n - 1) stride at or above 2^63, an unpack output that is not 16-byte aligned, pack's alignment rules, n too large for one launch's
  grid, every overlap: the code, a message, and the output untouched; n == 0 touches nothing;
* N = 1024 with n = 4097: the routed path's second pass through its pool block;
* a second identical he355_bfv_unpack_bytes_ntt makes no raw hipMalloc (the fused path, and N = 1024's pool block), and he355_bfv_route_stats
  says which of the two ran (and counts the two passes of n = 4097);
* end to end: n4096_d3, real keys, 16 records of Bmax random bytes, unpack_bytes_ntt at L_out = L_top, the query Enc(2^-4 X^i):
  expand(16) -> to_ntt -> bfv_multiply_plain_accumulate (1 x 1 x 16) -> from_ntt -> decrypt -> pack_bytes gives record i byte for byte, for
  two values of i; the noise budget is positive before the decryption."""

import numpy as np
import pytest

from bfv_bytes_ref import np_fields
from bfv_gpu_helpers import SENT, At, be, expand_keys, inner_of, pair, refused, sentinelled  # noqa: F401 (be: the fixture)

pytestmark = pytest.mark.gpu

N2048 = (2048, [60, 40, 60], 20)
W16 = (2048, [60, 40, 60], 17)
W21 = (2048, [60, 40, 60], 22)
CHAINS = ["n1024", N2048, "n4096_d3", W16, W21]
IDS = ["n1024", "n2048", "n4096_d3", "n2048_w16", "n2048_w21"]
BASE = 3  # the byte slab starts 3 bytes into its buffer


def byte_slab(g, rng, n, B, stride, base=BASE):
    """(device buffer, host image as uint8, data [n][B]): 0xFF everywhere but the n plaintexts of B bytes at base + j stride"""
    size = (base + (n - 1) * stride + B + 16 + 7) // 8 * 8
    img = np.full(size, 0xFF, dtype=np.uint8)
    data = rng.integers(0, 256, (n, B), dtype=np.uint8)
    data[:, B - 1] |= 0x80
    for j in range(n):
        img[base + j * stride: base + j * stride + B] = data[j]
    return g.to_device(img.view(np.uint64)), img, data


def byte_sizes(Bmax):
    return sorted({1, 9, Bmax - 1, Bmax})


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_unpack_and_pack(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(91)
    Bmax, w = g.bfv_bytes_per_plain()
    assert w == o.t.bit_length() - 1 and Bmax == N * w // 8
    for B in byte_sizes(Bmax):
        W8 = (B + 7) // 8 * 8
        for n in (1, 3):
            want = None
            for stride in (B, B + 5, W8 + 8):
                what = (B, n, stride)
                src, img, data = byte_slab(g, rng, n, B, stride)
                want = np_fields(data, w, N)
                out = sentinelled(g, n * N, N)
                g.bfv_unpack_bytes(n, src, BASE, stride, B, At(out, N))
                assert np.array_equal(inner_of(out, N, what).reshape(n, N), want), (what, "fields")
                assert np.array_equal(src.download().view(np.uint8), img), (what, "input")
                src.free()
                # the inverse, from the coefficients as they lie on the device and from words with junk above bit w
                junk = want | (rng.integers(0, 2 ** 63, want.shape, dtype=np.uint64) << np.uint64(w))
                dj = g.to_device(junk)
                for ps in (W8, W8 + 8):
                    for coef, name in ((At(out, N), "clean"), (dj, "junk")):
                        back = g.to_device(np.full((n * ps + 16) // 8, SENT, dtype=np.uint64))
                        g.bfv_pack_bytes(n, coef, B, ps, back, 8)
                        got = back.download()
                        exp = np.full(got.size, SENT, dtype=np.uint64).view(np.uint8)
                        for j in range(n):
                            exp[8 + j * ps: 8 + j * ps + W8] = 0
                            exp[8 + j * ps: 8 + j * ps + B] = data[j]
                        assert np.array_equal(got.view(np.uint8), exp), (what, ps, name)
                        back.free()
                assert np.array_equal(dj.download(want.shape), junk), (what, "pack's input")
                assert np.array_equal(inner_of(out, N, what).reshape(n, N), want), (what, "pack's input")
                dj.free()
                out.free()
    g.close()


def composition(g, L_out, n, src, base, stride, B, N):
    """the definition: he355_bfv_unpack_bytes, then he355_bfv_plain_to_ntt"""
    plain, ref = g.alloc(n * N), g.alloc(n * L_out * N)
    g.bfv_unpack_bytes(n, src, base, stride, B, plain)
    g.bfv_plain_to_ntt(L_out, n, plain, ref)
    out = ref.download((n, L_out, N))
    plain.free()
    ref.free()
    return out


@pytest.mark.parametrize("chain", CHAINS, ids=IDS)
def test_unpack_ntt_equals_the_composition(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(92)
    Bmax, w = g.bfv_bytes_per_plain()
    for L_out in sorted({g.L, 1}):
        for B in (9, Bmax):
            for n in (1, 3):
                what = (L_out, B, n)
                src, img, data = byte_slab(g, rng, n, B, B)
                want = composition(g, L_out, n, src, BASE, B, B, N)
                buf = sentinelled(g, n * L_out * N, N)
                g.bfv_unpack_bytes_ntt(L_out, n, src, BASE, B, B, At(buf, N))
                assert np.array_equal(inner_of(buf, N, what).reshape(n, L_out, N), want), what
                assert np.array_equal(src.download().view(np.uint8), img), (what, "input")
                src.free()
                buf.free()
    # behind an unsynchronised producer: the byte slab is still being copied when the call is queued
    L_out, n, B = g.L, 3, Bmax
    src, img, data = byte_slab(g, rng, n, B, B)
    dst, out = g.to_device(np.zeros(src.n, dtype=np.uint64)), g.alloc(n * L_out * N)
    g.sync()
    src.copy_into(dst)
    g.bfv_unpack_bytes_ntt(L_out, n, dst, BASE, B, B, out)
    got = out.download((n, L_out, N))
    assert np.array_equal(dst.download().view(np.uint8), img)
    assert np.array_equal(got, composition(g, L_out, n, src, BASE, B, B, N)), "producer"
    g.close()


def test_refusals(be, oracle):
    g, o, N, *_ = pair(be, oracle, "n4096_d3")
    rng = np.random.default_rng(93)
    L = g.L
    Bmax, w = g.bfv_bytes_per_plain()
    S = (Bmax + 7) // 8 * 8
    src, img, _ = byte_slab(g, rng, 2, Bmax, S, base=0)
    out = g.to_device(np.full(2 * L * N, SENT, dtype=np.uint64))
    bout = g.to_device(np.full(2 * S // 8 + 2, SENT, dtype=np.uint64))
    un = lambda n=2, buf=src, off=0, stride=S, B=Bmax, dst=out: g.bfv_unpack_bytes(n, buf, off, stride, B, dst)
    nt = lambda n=2, buf=src, off=0, stride=S, B=Bmax, dst=out, L_out=L: g.bfv_unpack_bytes_ntt(L_out, n, buf, off, stride, B, dst)
    pk = lambda n=2, buf=bout, off=0, stride=S, B=Bmax, dst=out: g.bfv_pack_bytes(n, dst, B, stride, buf, off)  # (dst: pack's INPUT)
    nmax = (2 ** 31 - 1) // (N // 256)
    for f in (un, nt, pk):
        refused(be, lambda: f(B=0))
        refused(be, lambda: f(B=Bmax + 1))
        refused(be, lambda: f(B=9, stride=8))
        refused(be, lambda: f(n=nmax + 1))
        refused(be, lambda: f(n=2 ** 40))
        f(n=0)
        refused(be, lambda: f(n=3, stride=2 ** 63))     # (n - 1) stride wraps to 0: the checked multiply, not the overlap test, refuses
        refused(be, lambda: f(n=2, stride=2 ** 63 - 8))  # (n - 1) stride + B reaches 2^63
    refused(be, lambda: un(dst=At(out, 1)))              # unpack stores two coefficients at once: a 16-byte aligned output
    refused(be, lambda: nt(L_out=0))
    refused(be, lambda: nt(L_out=L + 1))
    refused(be, lambda: pk(off=4))                       # the packed side is not 8-byte aligned
    refused(be, lambda: pk(stride=S + 4))                # its stride is no multiple of 8
    refused(be, lambda: pk(B=9, stride=8))               # nor may two plaintexts share a word
    # overlaps, inside one slab of 4 N words (every range named here lies inside it)
    slab = g.to_device(np.full(4 * N, SENT, dtype=np.uint64))
    refused(be, lambda: un(n=1, buf=slab, dst=slab))                                        # the same address
    refused(be, lambda: un(n=1, buf=slab, off=8 * N - 1, B=1, stride=1, dst=slab))            # the last byte of the output's range
    refused(be, lambda: un(n=2, buf=slab, off=8 * N - 5, B=1, stride=9, dst=At(slab, N)))     # only the second plaintext's byte lies inside
    refused(be, lambda: un(n=1, buf=slab, off=0, B=17, stride=17, dst=At(slab, 2)))           # the output starts inside the bytes
    refused(be, lambda: nt(n=1, buf=slab, off=8 * 2 * N - 1, B=1, stride=1, dst=slab, L_out=2))  # the output's range is L_out times as long
    refused(be, lambda: pk(n=1, buf=slab, off=8 * N - 8, B=1, stride=8, dst=slab))            # pack writes the WHOLE word: the input's last
    refused(be, lambda: pk(n=1, buf=slab, off=0, B=8, stride=8, dst=slab))
    assert (slab.download() == SENT).all()
    assert (out.download() == SENT).all() and (bout.download() == SENT).all()
    assert np.array_equal(src.download().view(np.uint8), img)
    g.close()
    ck = be.Context(be.SCHEME_CKKS, N, bit_sizes=[60, 40, 40, 60], sec128=False, device=0)
    a, b = ck.to_device(np.full(64, SENT, dtype=np.uint64)), ck.to_device(np.full(ck.L * N, SENT, dtype=np.uint64))
    refused(be, lambda: ck.bfv_unpack_bytes(1, a, 0, 8, 8, b))
    refused(be, lambda: ck.bfv_unpack_bytes_ntt(ck.L, 1, a, 0, 8, 8, b))
    refused(be, lambda: ck.bfv_pack_bytes(1, b, 8, 8, a))
    assert ck.bfv_bytes_per_plain() == (0, 0)
    assert (a.download() == SENT).all() and (b.download() == SENT).all()
    ck.close()


def test_n1024_second_pass_of_the_chunk_loop(be, oracle):
    """N = 1024 is routed through one pool block, 4096 plaintexts per pass: n = 4097 makes a second pass of ONE plaintext, which must read
    its bytes at 4096 stride and write at 4096 L_out N; the last plaintexts are held to numpy fields + he355_bfv_plain_to_ntt"""
    g, o, N, *_ = pair(be, oracle, "n1024")
    rng = np.random.default_rng(96)
    n, B, L_out, keep = 4097, 9, 1, 3
    src, img, data = byte_slab(g, rng, n, B, B)
    buf = sentinelled(g, n * L_out * N, N)
    g.bfv_route_stats(reset=True)
    g.bfv_unpack_bytes_ntt(L_out, n, src, BASE, B, B, At(buf, N))
    routes = {k: c for k, c in g.bfv_route_stats().items() if c}
    assert routes == {"bytes_routed": 2}, routes
    got = inner_of(buf, N, "chunks").reshape(n, L_out, N)
    Bmax, w = g.bfv_bytes_per_plain()
    plain, ref = g.to_device(np_fields(data[-keep:], w, N)), g.alloc(keep * L_out * N)
    g.bfv_plain_to_ntt(L_out, keep, plain, ref)
    assert np.array_equal(got[-keep:], ref.download((keep, L_out, N)))
    assert np.array_equal(got[:keep], composition(g, L_out, keep, src, BASE, B, B, N))
    assert np.array_equal(src.download().view(np.uint8), img)
    g.close()


@pytest.mark.parametrize("chain", ["n1024", "n4096_d3"])
def test_second_identical_unpack_ntt_makes_no_raw_allocation(be, oracle, chain):
    g, o, N, *_ = pair(be, oracle, chain)
    rng = np.random.default_rng(94)
    Bmax, w = g.bfv_bytes_per_plain()
    n = 3
    src, img, data = byte_slab(g, rng, n, Bmax, Bmax)
    out = g.alloc(n * g.L * N)
    g.bfv_unpack_bytes_ntt(g.L, n, src, BASE, Bmax, Bmax, out)
    g.sync()
    first = g.alloc_stats()
    g.bfv_route_stats(reset=True)
    g.bfv_unpack_bytes_ntt(g.L, n, src, BASE, Bmax, Bmax, out)
    g.sync()
    second = g.alloc_stats()
    assert second["raw_mallocs"] == first["raw_mallocs"] and second["raw_frees"] == first["raw_frees"], (first, second)
    routes = {k: c for k, c in g.bfv_route_stats().items() if c}  # N = 1024 has no column pass: one pass of the composition
    assert routes == ({"bytes_routed": 1} if N == 1024 else {"bytes_fused": 1}), routes
    assert np.array_equal(out.download((n, g.L, N)), composition(g, g.L, n, src, BASE, Bmax, Bmax, N))
    g.close()


def test_end_to_end_retrieval_of_byte_records(be, oracle):
    count, idx = 16, [11, 0]
    n = len(idx)
    g, o, N, sk, pk = pair(be, oracle, "n4096_d3", keys=True)
    expand_keys(g, o, sk, count, 260)
    L, t = g.L, o.t
    Bmax, w = g.bfv_bytes_per_plain()
    rng = np.random.default_rng(95)
    records = rng.integers(0, 256, (count, Bmax), dtype=np.uint8)
    records[11, :4] = [0, 0xFF, 0x80, 1]
    img = np.zeros((count * Bmax + 7) // 8 * 8, dtype=np.uint8)
    img[:count * Bmax] = records.reshape(-1)
    dbn = g.alloc(count * L * N)
    g.bfv_unpack_bytes_ntt(L, count, g.to_device(img.view(np.uint64)), 0, Bmax, Bmax, dbn)      # the database as it lies, contiguous
    qp = np.zeros((n, N), dtype=np.uint64)
    for r, i in enumerate(idx):
        qp[r, i] = pow(16, -1, t)
    per = 2 * L * N
    query, kids = g.alloc(n * per), g.alloc(count * n * per)
    g.encrypt(n, g.to_device(qp), 95, 0, query)
    g.bfv_expand(L, n, query, count, kids)                                                   # child k of query r at k n + r
    g.bfv_transform_to_ntt(L, 2, count * n, kids, kids)
    res = g.alloc(n * per)
    for r in range(n):
        g.bfv_multiply_plain_accumulate(L, 2, 1, 1, count, At(kids, r * per), 1, n, dbn, 1, 1, At(res, r * per))
    g.bfv_transform_from_ntt(L, 2, n, res, res)
    budget = g.bfv_noise_budget(L, 2, n, res)
    print("byte-record retrieval: noise budget before the decryption (bits)", budget.min(), "..", budget.max())
    assert (budget > 0).all(), budget
    plain = g.alloc(n * N)
    g.decrypt(L, 2, n, res, plain)
    S = (Bmax + 7) // 8 * 8
    back = g.alloc(n * S // 8)
    g.bfv_pack_bytes(n, plain, Bmax, S, back)
    got = back.download().view(np.uint8).reshape(n, S)
    for r, i in enumerate(idx):
        assert np.array_equal(got[r, :Bmax], records[i]), i
        assert (got[r, Bmax:] == 0).all()
    g.close()
