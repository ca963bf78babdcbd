"""The references of the hoisted rotation family (tests/rotate_hoisted_ref.py, rotate_hoisted_lazy_ref.py, linear_transform_bsgs_ref.py) on
every layout of tests/hoisted_layouts.py, without a device: what tests/test_gpu_hoisted_layouts.py holds the kernels to is itself held,
on the same chains, to anchors that do not go through its own arithmetic.  Per layout, at L_top and L = 1 (deep_4096: L = 2 as well), one
ciphertext, bit for bit:

* the lazy sum of ONE keyed step under the all-ones plaintext (Python integers, one mod-down) is rotate_hoisted_ref.hoisted (the oracle's
  key switch under the permuted key, then sigma): P is odd, so the mod-down commutes with sigma;
* the transform with one identity giant row is the lazy sum over its baby steps (mod_down(A + P B) = B + mod_down(A));
* CKKS: at c1 = 0 `hoisted` is (sigma_g(c0), 0) whatever the key, at g = N + 1, N - 1, 3, 2N - 3, 5^(N/4) and 2N - 1.
BFV layouts run NTT-form residues, as the lazy sum and the transform do on the device.  No GPU, no backend."""
import zlib

import numpy as np
import pytest

import hoisted_layouts as hl
import linear_transform_bsgs_ref as bsgs
import rotate_hoisted_lazy_ref as lazy
import rotate_hoisted_ref as ref


def _rng(name, salt):
    return np.random.default_rng(zlib.crc32((salt + name).encode()))


@pytest.mark.parametrize("name", list(hl.LAYOUTS))
def test_the_anchors_hold_on_every_layout(oracle, name):
    o = hl.make_oracle(oracle, name)
    rng = _rng(name, "anchors")
    e3 = o.galois_elt(3)
    keys = {e3: o.random_kswitch_key(rng), o.galois_elt(1): o.random_kswitch_key(rng)}
    for L in hl.levels(name, o.L):
        ct = o.random_poly(rng, L, 2)
        got = lazy.plain_sum_lazy(o, ct[None], [3], keys, lazy.ones_qp(o, L)[None])[0]
        assert np.array_equal(got, ref.hoisted(o, ct, e3, keys[e3], 1)), (name, L, "the lazy sum of one step under ones is the eager rotation")
        baby = [0, 1, 3]
        plains = np.stack([o.random_poly(rng, L, 1, special=True)[0] for _ in baby])
        got = bsgs.linear_transform_bsgs(o, ct[None], baby, [0], keys, plains[None])[0]
        assert np.array_equal(got, lazy.plain_sum_lazy(o, ct[None], baby, keys, plains)[0]), (name, L, "one identity giant row is the lazy sum")


@pytest.mark.parametrize("name", hl.CKKS)
def test_ckks_closed_form_at_c1_zero(oracle, name):
    o = hl.make_oracle(oracle, name)
    rng = _rng(name, "closed form")
    key = o.random_kswitch_key(rng)
    for L in hl.levels(name, o.L):
        ct = o.random_poly(rng, L, 2)
        ct[1] = 0
        for g in hl.closed_form_elts(o.N):
            got = ref.hoisted(o, ct, g, key, 1)
            assert not got[1].any(), (name, L, g)
            for j in range(L):
                assert np.array_equal(got[0, j], o.apply_galois_poly(j, g, 1, ct[0, j])), (name, L, g, j)


def test_the_table_holds_the_paths_it_names():
    assert len(hl.CKKS) == 19 and len(hl.BFV) == 8
    shoup_large = {k for k in hl.LAYOUTS if hl.entry(k)["form"] == "shoup" and hl.entry(k)["N"] >= 8192}  # the Shoup build from N = 8192
    assert shoup_large == {"n8192_shoup", "n16384_shoup", "n32768_shoup", "bfv_n16384_shoup"}
    for name in hl.LAYOUTS:
        e = hl.entry(name)
        assert e["N"] in (1024, 2048, 4096, 8192, 16384, 32768) and len(e["bits"]) >= 3 and e["for"], name
    fp64 = lambda name: hl.engines(hl.entry(name)["primes"])[0]
    assert fp64("unsorted_small_special")[-1] and not fp64("tiny")[-1]
    assert set(hl.EDGED) == {"f64_only_1024", "f64_only_4096", "f64_only_32768", "tiny", "tiny_n1024", "unsorted_small_special",
                             "unsorted_small_special_n1024", "fold_max_c_x7"}
