"""MI355X-native HEBench backend — Python loader for the C ABI (include/he355.h).

The product is the shared library ``lib/libhebench_mi355x_backend.so`` (HIP kernels + C++17 host + the
HEBench API-Bridge entry points).  This module only binds its C ABI with ctypes so that tests, ``bench.py``
and ``__graft_entry__`` can drive it; it contains no arithmetic and never imports ``oracle``.

Import with ``importlib.import_module("reference-seal-backend_amd")`` (the directory name has a hyphen).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HE355_LIB_PATH selects another build of the same library (A/B timing of kernel variants, sanitizer builds): the product
# file is never swapped in place
LIB_PATH = os.environ.get("HE355_LIB_PATH") or os.path.join(_HERE, "lib", "libhebench_mi355x_backend.so")

SCHEME_BFV, SCHEME_CKKS = 1, 2
OK, E_INVALID_ARGS, E_PARAMS, E_DEVICE = 0, 1, 2, 3


class HE355Error(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"he355 error {code}: {msg}")
        self.code = code


class Indexer(C.Structure):
    _fields_ = [("a_base", C.c_uint64), ("b_base", C.c_uint64), ("b1", C.c_uint64),
                ("pairwise", C.c_int32), ("reserved", C.c_int32)]


class AllocStats(C.Structure):
    _fields_ = [("raw_mallocs", C.c_uint64), ("raw_frees", C.c_uint64), ("pool_hits", C.c_uint64), ("pool_misses", C.c_uint64),
                ("cached_bytes", C.c_uint64), ("live_bytes", C.c_uint64)]


class PathStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("ks_fused", "ks_unfused", "ks_latency", "ks_lds", "level_sums_in_k3", "level_sums_by_kernel",
                                           "level_sum_launches_in_k3", "reserved")]


class HoistStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("digit_lifts", "key_products", "keys_permuted", "key_bytes", "mod_downs", "inner_sums")] + [("reserved", C.c_uint64 * 2)]


class PolyStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("combinations", "products", "rescales", "drops", "adds", "chunks", "calls", "complex_combinations")]


class RaiseStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("calls", "chunks", "fused_launches", "streaming_launches", "split_launches")] + [("reserved", C.c_uint64 * 3)]


class ChebStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("calls", "chunks", "products", "fused_steps", "combinations", "drops", "adds", "double_angles")]


class PolyPlan(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("depth", "L_out", "min_scalar_bits", "degree")]
                + [(k, C.c_uint64) for k in ("products", "combinations", "rescales", "drops", "adds", "powers", "chunks", "pool_bytes")]
                + [("out_scale", C.c_double), ("power_mask", C.c_uint64 * 16), ("reserved", C.c_uint64 * 5)])


class Term(C.Structure):
    _fields_ = [("d_ct", C.c_void_p), ("L", C.c_int32), ("reserved", C.c_int32)]


class BfvRouteStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("cut_cols", "cut_stream", "mac_gadget", "mac_plain", "own_cols", "own_stream", "digits_fused",
                                           "digits_routed", "bytes_fused", "bytes_routed", "passes", "select_cols", "select_stream",
                                           "select_tail_fused", "select_tail_routed")] + [("reserved", C.c_uint64 * 1)]


class BfvMultiplyStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("calls_lists", "calls_pairs", "chunks", "cols_fused", "cols_unfused", "cols_exact", "coef_wide",
                                           "rows_dual", "rows_split", "inv_dual", "inv_split", "lds_limit")] + [("reserved", C.c_uint64 * 4)]


def build(force: bool = False) -> str:
    """Compile the backend for gfx950 with hipcc (csrc/Makefile)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.run(["make", "-C", csrc, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", csrc, "-j8", "-s"], check=True)
    return LIB_PATH


_lib = None
_u64p = C.POINTER(C.c_uint64)


def lib():
    """The loaded shared library.  Fails loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no fallback path)")
        L = C.CDLL(LIB_PATH)
        vp, u64, i32, u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32
        vpp = C.POINTER(vp)
        u8p = C.POINTER(C.c_uint8)
        sig = {
            "he355_last_error": (C.c_char_p, []),
            "he355_ctx_create": (i32, [i32, u64, C.POINTER(C.c_int32), u64, i32, i32, vpp]),
            "he355_ctx_create_primes": (i32, [i32, u64, _u64p, u64, u64, vpp]),
            "he355_ctx_destroy": (None, [vp]),
            "he355_poly_degree": (u64, [vp]), "he355_key_modulus_count": (u64, [vp]),
            "he355_data_modulus_count": (u64, [vp]), "he355_modulus": (u64, [vp, u64]),
            "he355_plain_modulus": (u64, [vp]), "he355_prime_uses_fp64": (i32, [vp, u64]),
            "he355_bfv_aux_base": (u64, [vp, i32, _u64p, u64]),
            "he355_galois_elt_from_step": (u32, [vp, i32]),
            "he355_galois_elts_all": (u64, [vp, C.POINTER(u32), u64]),
            "he355_device_count": (i32, [C.POINTER(i32)]),
            "he355_device_init": (i32, [vp, i32]),
            "he355_malloc": (i32, [vp, u64, vpp]), "he355_free": (i32, [vp, vp]),
            "he355_upload": (i32, [vp, vp, vp, u64]), "he355_download": (i32, [vp, vp, vp, u64]),
            "he355_copy": (i32, [vp, vp, vp, u64]),
            "he355_copy_peer": (i32, [vp, vp, vp, vp, u64]),
            "he355_sync": (i32, [vp]),
            "he355_fill_uniform": (i32, [vp, vp, u64, u8p, u32, u64]),
            "he355_fill_uniform_at": (i32, [vp, vp, u64, u8p, u32, u64, u64]),
            "he355_set_dual_stream": (i32, [vp, i32]),
            "he355_set_relin_key": (i32, [vp, _u64p]), "he355_set_galois_key": (i32, [vp, u32, _u64p]),
            "he355_set_relin_key_synthetic": (i32, [vp, u64]),
            "he355_set_galois_key_synthetic": (i32, [vp, u32, u64]),
            "he355_add": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_sub": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_multiply": (i32, [vp, i32, u64, vp, vp, Indexer, vp]),
            "he355_bfv_multiply": (i32, [vp, i32, u64, vp, vp, Indexer, vp]),
            "he355_multiply_relin": (i32, [vp, i32, u64, vp, vp, Indexer, i32, vp]),
            "he355_relinearize": (i32, [vp, i32, u64, vp, vp]),
            "he355_relinearize_rescale": (i32, [vp, i32, u64, vp, vp]),
            "he355_set_public_key": (i32, [vp, vp]), "he355_set_secret_key": (i32, [vp, vp]),
            "he355_encrypt": (i32, [vp, u64, vp, u64, u64, vp]),
            "he355_keygen_relin": (i32, [vp, u64]), "he355_keygen_galois": (i32, [vp, C.c_uint32, u64]),
            "he355_ckks_encode": (i32, [vp, u64, vp, u64, C.c_double, vp]),
            "he355_ckks_decode": (i32, [vp, i32, u64, vp, C.c_double, vp]),
            "he355_bfv_encode": (i32, [vp, u64, vp, u64, vp]),
            "he355_bfv_decode": (i32, [vp, u64, vp, vp]),
            "he355_ckks_decode_slots": (i32, [vp, i32, u64, vp, C.c_double, _u64p, u64, vp]),
            "he355_bfv_decode_slots": (i32, [vp, u64, vp, _u64p, u64, vp]),
            "he355_host_alloc": (i32, [vp, u64, vpp]), "he355_host_free": (i32, [vp, vp]),
            "he355_decrypt": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_multiply_plain": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_add_plain": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_mod_switch_drop": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_bfv_mod_switch": (i32, [vp, i32, i32, i32, u64, vp, vp]),
            "he355_bfv_add_plain": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_bfv_sub_plain": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_bfv_multiply_plain": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_bfv_noise_budget": (i32, [vp, i32, i32, u64, vp, vp, vp]),
            "he355_bfv_transform_to_ntt": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_bfv_transform_from_ntt": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_bfv_plain_to_ntt": (i32, [vp, i32, u64, vp, vp]),
            "he355_bfv_multiply_plain_ntt": (i32, [vp, i32, i32, u64, vp, vp, Indexer, vp]),
            "he355_bfv_multiply_plain_accumulate": (i32, [vp, i32, i32, u64, u64, u64, vp, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_multiply_monomial": (i32, [vp, i32, i32, u64, vp, u32, vp]),
            "he355_bfv_expand_galois_elts": (u64, [vp, u64, C.POINTER(u32), u64]),
            "he355_bfv_expand": (i32, [vp, i32, u64, vp, u64, vp]),
            "he355_bfv_merge": (i32, [vp, i32, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_digit_count": (u64, [vp, i32, C.POINTER(u32), u64]),
            "he355_bfv_decompose": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_bfv_decompose_ntt": (i32, [vp, i32, i32, u64, vp, i32, vp]),
            "he355_bfv_compose": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_bfv_gadget_count": (u64, [vp, i32, i32, C.POINTER(u32), u64]),
            "he355_bfv_gadget_decompose": (i32, [vp, i32, i32, i32, u64, vp, vp]),
            "he355_bfv_gadget_decompose_ntt": (i32, [vp, i32, i32, i32, u64, vp, vp]),
            "he355_bfv_rgsw_encrypt": (i32, [vp, i32, i32, u64, vp, u64, u64, vp]),
            "he355_bfv_external_product": (i32, [vp, i32, i32, u64, u64, vp, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_select": (i32, [vp, i32, i32, u64, u64, vp, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_selector_encrypt": (i32, [vp, i32, i32, u64, u64, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_rgsw_encrypt_secret": (i32, [vp, i32, i32, u64, u64, vp]),
            "he355_bfv_rgsw_from_bfv": (i32, [vp, i32, i32, i32, u64, u64, vp, u64, u64, vp, vp]),
            "he355_bfv_bytes_per_plain": (u64, [vp, C.POINTER(u32)]),
            "he355_bfv_unpack_bytes": (i32, [vp, u64, vp, u64, u64, vp]),
            "he355_bfv_unpack_bytes_ntt": (i32, [vp, i32, u64, vp, u64, u64, vp]),
            "he355_bfv_pack_bytes": (i32, [vp, u64, vp, u64, u64, vp]),
            "he355_bfv_reply_bytes": (u64, [vp, i32, i32]),
            "he355_bfv_reply_safe_bits": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
            "he355_bfv_reply_compress": (i32, [vp, i32, i32, i32, u64, vp, vp, u64]),
            "he355_bfv_reply_decrypt": (i32, [vp, i32, i32, u64, vp, u64, vp, vp, vp]),
            "he355_bfv_seeded_encrypt": (i32, [vp, i32, u64, vp, u64, u64, u64, vp]),
            "he355_bfv_seeded_selector_encrypt": (i32, [vp, i32, i32, u64, u64, u64, u64, vp, u64, u64, u64, vp]),
            "he355_bfv_seeded_restore": (i32, [vp, i32, i32, u64, vp, u64, u64, vp]),
            "he355_keygen_galois_seeded": (i32, [vp, u32, u64, u64, vp]),
            "he355_set_galois_key_seeded": (i32, [vp, u32, _u64p, u64]),
            "he355_sum": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_multiply_accumulate": (i32, [vp, i32, u64, u64, u64, vp, u64, u64, vp, u64, u64, vp]),
            "he355_bfv_multiply_relin_accumulate": (i32, [vp, i32, u64, u64, u64, vp, u64, u64, vp, u64, u64, vp]),
            "he355_rescale": (i32, [vp, i32, i32, u64, vp, vp]),
            "he355_apply_galois": (i32, [vp, i32, u64, vp, u32, vp]),
            "he355_rotate": (i32, [vp, i32, u64, vp, i32, vp]),
            "he355_rotate_add": (i32, [vp, i32, u64, vp, i32, vp, vp]),
            "he355_rotate_each": (i32, [vp, i32, u64, vp, vp, vp]),
            "he355_rotate_sum": (i32, [vp, i32, u64, vp, vp, u64, vp, vp]),
            "he355_accumulate": (i32, [vp, i32, u64, vp, u64, vp]),
            "he355_apply_galois_hoisted": (i32, [vp, i32, i32, u64, vp, C.POINTER(u32), u64, vp]),
            "he355_rotate_hoisted": (i32, [vp, i32, i32, u64, vp, C.POINTER(C.c_int32), u64, vp]),
            "he355_rotate_hoisted_plain_sum": (i32, [vp, i32, u64, vp, C.POINTER(C.c_int32), u64, vp, vp]),
            "he355_rotate_hoisted_plain_sum_lazy": (i32, [vp, i32, u64, vp, C.POINTER(C.c_int32), u64, vp, vp]),
            "he355_plain_extend_special": (i32, [vp, i32, u64, vp, vp, vp]),
            "he355_linear_transform_bsgs": (i32, [vp, i32, u64, vp, C.POINTER(C.c_int32), u64, C.POINTER(C.c_int32), u64, vp, C.POINTER(C.c_uint8), vp]),
            "he355_linear_transform_bsgs_scratch_bytes": (u64, [vp, i32, u64, u64]),
            "he355_hoist_stats": (i32, [vp, C.POINTER(HoistStats), i32]),
            "he355_hoist_release_keys": (i32, [vp]),
            "he355_combine_scalars": (i32, [vp, i32, i32, u64, C.POINTER(Term), u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]),
            "he355_ckks_scalar_residues": (i32, [vp, i32, C.c_double, C.POINTER(C.c_uint64)]),
            "he355_ckks_eval_poly_plan": (i32, [vp, i32, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, u64, C.POINTER(PolyPlan)]),
            "he355_ckks_eval_poly": (i32, [vp, i32, u64, vp, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, vp]),
            "he355_poly_stats": (i32, [vp, C.POINTER(PolyStats), i32]),
            "he355_ckks_encode_complex": (i32, [vp, u64, vp, u64, C.c_double, vp]),
            "he355_ckks_decode_complex": (i32, [vp, i32, u64, vp, C.c_double, vp]),
            "he355_ckks_decode_complex_slots": (i32, [vp, i32, u64, vp, C.c_double, _u64p, u64, vp]),
            "he355_ckks_complex_unit": (i32, [vp, i32, C.POINTER(C.c_uint64)]),
            "he355_ckks_complex_scalar_residues": (i32, [vp, i32, C.c_double, C.c_double, C.POINTER(C.c_uint64)]),
            "he355_combine_scalars_complex": (i32, [vp, i32, i32, u64, C.POINTER(Term), u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]),
            "he355_ckks_eval_poly_complex_plan": (i32, [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, u64, C.POINTER(PolyPlan)]),
            "he355_ckks_eval_poly_complex": (i32, [vp, i32, u64, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, vp]),
            "he355_ckks_mod_raise": (i32, [vp, i32, i32, i32, u64, vp, vp]),
            "he355_ckks_lift_centred": (i32, [vp, i32, u64, vp, vp]),
            "he355_raise_stats": (i32, [vp, C.POINTER(RaiseStats), i32]),
            "he355_combine_scalars_rescale": (i32, [vp, i32, i32, u64, C.POINTER(Term), u64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]),
            "he355_ckks_eval_chebyshev_plan": (i32, [vp, i32, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, u64, C.POINTER(PolyPlan)]),
            "he355_ckks_eval_chebyshev": (i32, [vp, i32, u64, vp, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, vp]),
            "he355_ckks_eval_mod_plan": (i32, [vp, i32, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, i32, u64, C.POINTER(PolyPlan)]),
            "he355_ckks_eval_mod": (i32, [vp, i32, u64, vp, C.POINTER(C.c_double), u64, i32, C.c_double, C.c_double, i32, vp]),
            "he355_cheb_stats": (i32, [vp, C.POINTER(ChebStats), i32]),
            "he355_encrypt_zero": (i32, [vp, u64, u64, u64, vp]),
            "he355_set_zero_stream": (i32, [vp, u64, u64]),
            "he355_ntt_forward": (i32, [vp, vp, u64, u8p, u32]),
            "he355_ntt_inverse": (i32, [vp, vp, u64, u8p, u32]),
            "he355_timer_begin": (i32, [vp]), "he355_timer_end": (i32, [vp, C.POINTER(C.c_float)]),
            "he355_probe_dominant_kernel": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
            "he355_clock_probe_begin": (i32, [vp, u64]), "he355_clock_probe_end": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
            "he355_set_chunk": (i32, [vp, u64]),
            "he355_set_latency_max": (i32, [vp, u64]),
            "he355_set_level_walk": (i32, [vp, i32]),
            "he355_set_lds_max": (i32, [vp, u64]),
            "he355_mem_info": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
            "he355_alloc_stats": (i32, [vp, C.POINTER(AllocStats)]),
            "he355_pool_trim": (i32, [vp, C.POINTER(C.c_uint64)]),
            "he355_path_stats": (i32, [vp, C.POINTER(PathStats), i32]),
            "he355_bfv_route_stats": (i32, [vp, C.POINTER(BfvRouteStats), i32]),
            "he355_bfv_multiply_stats": (i32, [vp, C.POINTER(BfvMultiplyStats), i32]),
            "he355_bridge_abi": (u64, [C.c_char_p, u64]),
            "he355_bridge_group_load_bytes": (u64, [i32, i32]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


C_ABI_SYMBOLS = [
    "he355_last_error", "he355_ctx_create", "he355_ctx_create_primes", "he355_ctx_destroy", "he355_poly_degree",
    "he355_key_modulus_count", "he355_data_modulus_count", "he355_modulus", "he355_plain_modulus",
    "he355_prime_uses_fp64", "he355_bfv_aux_base", "he355_galois_elt_from_step", "he355_galois_elts_all", "he355_device_count",
    "he355_device_init", "he355_malloc", "he355_free", "he355_upload", "he355_download", "he355_copy", "he355_copy_peer", "he355_sync",
    "he355_fill_uniform", "he355_fill_uniform_at", "he355_set_dual_stream", "he355_set_relin_key", "he355_set_galois_key", "he355_set_relin_key_synthetic",
    "he355_set_galois_key_synthetic", "he355_add", "he355_sub", "he355_multiply", "he355_bfv_multiply", "he355_multiply_relin",
    "he355_relinearize", "he355_relinearize_rescale", "he355_multiply_accumulate", "he355_bfv_multiply_relin_accumulate", "he355_multiply_plain", "he355_add_plain",
    "he355_mod_switch_drop", "he355_bfv_mod_switch", "he355_bfv_add_plain", "he355_bfv_sub_plain", "he355_bfv_multiply_plain", "he355_bfv_noise_budget", "he355_bfv_transform_to_ntt", "he355_bfv_transform_from_ntt", "he355_bfv_plain_to_ntt",
    "he355_bfv_multiply_plain_ntt", "he355_bfv_multiply_plain_accumulate", "he355_bfv_multiply_monomial", "he355_bfv_expand_galois_elts", "he355_bfv_expand", "he355_bfv_merge", "he355_bfv_digit_count", "he355_bfv_decompose", "he355_bfv_decompose_ntt", "he355_bfv_compose", "he355_bfv_gadget_count", "he355_bfv_gadget_decompose", "he355_bfv_gadget_decompose_ntt", "he355_bfv_rgsw_encrypt", "he355_bfv_external_product", "he355_bfv_select", "he355_bfv_selector_encrypt", "he355_bfv_rgsw_encrypt_secret", "he355_bfv_rgsw_from_bfv", "he355_bfv_bytes_per_plain", "he355_bfv_unpack_bytes", "he355_bfv_unpack_bytes_ntt", "he355_bfv_pack_bytes", "he355_bfv_reply_bytes", "he355_bfv_reply_safe_bits", "he355_bfv_reply_compress", "he355_bfv_reply_decrypt", "he355_bfv_seeded_encrypt", "he355_bfv_seeded_selector_encrypt", "he355_bfv_seeded_restore", "he355_keygen_galois_seeded", "he355_set_galois_key_seeded", "he355_sum", "he355_set_public_key", "he355_set_secret_key", "he355_encrypt", "he355_decrypt", "he355_keygen_relin", "he355_keygen_galois", "he355_ckks_encode", "he355_ckks_decode",
    "he355_bfv_encode", "he355_bfv_decode", "he355_ckks_decode_slots", "he355_bfv_decode_slots", "he355_host_alloc", "he355_host_free", "he355_rescale", "he355_apply_galois", "he355_rotate", "he355_rotate_add", "he355_rotate_each", "he355_rotate_sum", "he355_accumulate", "he355_apply_galois_hoisted", "he355_rotate_hoisted", "he355_rotate_hoisted_plain_sum", "he355_rotate_hoisted_plain_sum_lazy", "he355_plain_extend_special", "he355_linear_transform_bsgs", "he355_linear_transform_bsgs_scratch_bytes", "he355_hoist_stats", "he355_hoist_release_keys", "he355_combine_scalars", "he355_ckks_scalar_residues", "he355_ckks_eval_poly_plan", "he355_ckks_eval_poly", "he355_poly_stats", "he355_ckks_encode_complex", "he355_ckks_decode_complex", "he355_ckks_decode_complex_slots", "he355_ckks_complex_unit", "he355_ckks_complex_scalar_residues", "he355_combine_scalars_complex", "he355_ckks_eval_poly_complex_plan", "he355_ckks_eval_poly_complex", "he355_ckks_mod_raise", "he355_ckks_lift_centred", "he355_raise_stats", "he355_combine_scalars_rescale", "he355_ckks_eval_chebyshev_plan", "he355_ckks_eval_chebyshev", "he355_ckks_eval_mod_plan", "he355_ckks_eval_mod", "he355_cheb_stats", "he355_encrypt_zero", "he355_set_zero_stream",
    "he355_ntt_forward", "he355_ntt_inverse", "he355_timer_begin", "he355_timer_end", "he355_probe_dominant_kernel", "he355_clock_probe_begin", "he355_clock_probe_end", "he355_set_chunk", "he355_set_latency_max", "he355_set_level_walk", "he355_set_lds_max", "he355_mem_info", "he355_alloc_stats", "he355_pool_trim", "he355_path_stats", "he355_bfv_route_stats", "he355_bfv_multiply_stats", "he355_bridge_abi", "he355_bridge_group_load_bytes",
]


def _check(code: int):
    if code != 0:
        raise HE355Error(code, lib().he355_last_error().decode())


def chain_bits(depth: int, coeff_bits: int) -> list[int]:
    """{60, bits x (depth-1), 60}: the reference's rule (seal_context.cpp:79-82,107-110)."""
    return [60] + [coeff_bits] * (depth - 1) + [60]


class DeviceBuffer:
    """A slab of uint64 in HBM owned by a Context."""

    def __init__(self, ctx: "Context", n_u64: int):
        self.ctx, self.n = ctx, int(n_u64)
        p = C.c_void_p()
        _check(lib().he355_malloc(ctx.h, self.n * 8, C.byref(p)))
        self.ptr = p

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr, dtype=np.uint64)
        assert a.size == self.n, (a.size, self.n)
        _check(lib().he355_upload(self.ctx.h, self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return self

    def download(self, shape=None) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint64)
        _check(lib().he355_download(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out.reshape(shape) if shape is not None else out

    def download_range(self, offset_u64: int, shape) -> np.ndarray:
        """prod(shape) elements starting at element offset_u64 (one row out of the middle or the end of a large slab)"""
        k = int(np.prod(shape))
        assert 0 <= offset_u64 and offset_u64 + k <= self.n, (offset_u64, k, self.n)
        out = np.empty(k, dtype=np.uint64)
        if k:
            _check(lib().he355_download(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr.value + int(offset_u64) * 8), out.nbytes))
        return out.reshape(shape)

    def download_head(self, shape) -> np.ndarray:
        """the first prod(shape) elements only (a sample of a large slab without moving the whole slab over PCIe)"""
        k = int(np.prod(shape))
        assert 0 <= k <= self.n, (k, self.n)
        out = np.empty(k, dtype=np.uint64)
        if k:
            _check(lib().he355_download(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out.reshape(shape)

    def copy_into(self, dst: "DeviceBuffer", dst_offset_u64: int = 0, n_u64: int | None = None):
        """device-to-device copy of the first n_u64 words of this slab to dst[dst_offset_u64:] (on the context's stream)"""
        n = self.n if n_u64 is None else int(n_u64)
        assert n <= self.n and dst_offset_u64 + n <= dst.n
        _check(lib().he355_copy(self.ctx.h, C.c_void_p(dst.ptr.value + dst_offset_u64 * 8), self.ptr, n * 8))

    def free(self):
        if self.ptr:
            lib().he355_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """Host mirror of the reference's SEALContextWrapper for the hot path: parameters + device state."""

    def __init__(self, scheme: int, N: int, bit_sizes=None, primes=None, plain_bits: int = 0,
                 plain_modulus: int = 0, sec128: bool = True, device: int | None = None):
        L = lib()
        h = C.c_void_p()
        if primes is not None:
            arr = np.asarray(primes, dtype=np.uint64)
            _check(L.he355_ctx_create_primes(scheme, N, arr.ctypes.data_as(_u64p), len(arr), plain_modulus, C.byref(h)))
        else:
            bs = (C.c_int32 * len(bit_sizes))(*bit_sizes)
            _check(L.he355_ctx_create(scheme, N, bs, len(bit_sizes), plain_bits, int(sec128), C.byref(h)))
        self.h = h
        self.scheme, self.N = scheme, N
        self.K = L.he355_key_modulus_count(h)
        self.L = L.he355_data_modulus_count(h)
        self.moduli = [L.he355_modulus(h, i) for i in range(self.K)]
        self.fp64 = [bool(L.he355_prime_uses_fp64(h, i)) for i in range(self.K)]
        self.t = L.he355_plain_modulus(h)
        self._bufs = []
        if device is not None:
            self.device_init(device)

    def bfv_aux_base(self, level: int | None = None) -> list[int]:
        """[m_sk, B_0, B_1, ...]: the auxiliary base of the BEHZ multiply at `level` data primes (host-side; no device needed)."""
        out = np.zeros(64, dtype=np.uint64)
        n = lib().he355_bfv_aux_base(self.h, self.L if level is None else level, out.ctypes.data_as(_u64p), 64)
        return [int(v) for v in out[:n]]

    def device_init(self, device: int = 0):
        _check(lib().he355_device_init(self.h, device))

    def close(self):
        if self.h:
            for b in self._bufs:
                b.free()
            self._bufs = []
            lib().he355_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- memory ----------------------------------------------------------------------------------
    def alloc(self, n_u64: int) -> DeviceBuffer:
        b = DeviceBuffer(self, n_u64)
        self._bufs.append(b)
        return b

    def to_device(self, arr: np.ndarray) -> DeviceBuffer:
        return self.alloc(arr.size).upload(arr)

    def fill_uniform(self, buf: DeviceBuffer, n_polys: int, prime_of, seed: int, first_poly: int = 0):
        pm = (C.c_uint8 * len(prime_of))(*prime_of)
        _check(lib().he355_fill_uniform_at(self.h, buf.ptr, n_polys, pm, len(prime_of), seed, first_poly))

    def set_dual_stream(self, on: bool):
        _check(lib().he355_set_dual_stream(self.h, int(on)))

    def sync(self):
        _check(lib().he355_sync(self.h))

    def set_chunk(self, ops: int):
        _check(lib().he355_set_chunk(self.h, ops))

    # -- keys ------------------------------------------------------------------------------------
    def set_relin_key(self, key: np.ndarray):
        k = np.ascontiguousarray(key, dtype=np.uint64)
        assert k.size == self.L * 2 * self.K * self.N
        _check(lib().he355_set_relin_key(self.h, k.ctypes.data_as(_u64p)))

    def set_galois_key(self, elt: int, key: np.ndarray):
        k = np.ascontiguousarray(key, dtype=np.uint64)
        assert k.size == self.L * 2 * self.K * self.N
        _check(lib().he355_set_galois_key(self.h, elt, k.ctypes.data_as(_u64p)))

    def keygen_relin(self, seed: int):
        _check(lib().he355_keygen_relin(self.h, seed))

    def keygen_galois(self, elt: int, seed: int):
        _check(lib().he355_keygen_galois(self.h, elt, seed))

    def set_relin_key_synthetic(self, seed: int):
        _check(lib().he355_set_relin_key_synthetic(self.h, seed))

    def set_galois_key_synthetic(self, elt: int, seed: int):
        _check(lib().he355_set_galois_key_synthetic(self.h, elt, seed))

    def galois_elt(self, step: int) -> int:
        return lib().he355_galois_elt_from_step(self.h, step)

    def galois_elts_all(self):
        buf = (C.c_uint32 * 64)()
        n = lib().he355_galois_elts_all(self.h, buf, 64)
        return [int(x) for x in buf[:n]]

    # -- evaluator (device slabs) ----------------------------------------------------------------
    @staticmethod
    def outer(a_base: int, b0: int, b_base: int, b1: int) -> Indexer:
        """HEBench indexers: result r = i*b1 + x uses operand0[a_base+i], operand1[b_base+x]."""
        return Indexer(a_base, b_base, b1, 0, 0)

    @staticmethod
    def pairwise(a_base: int = 0, b_base: int = 0) -> Indexer:
        return Indexer(a_base, b_base, 1, 1, 0)

    def add(self, L, size, n, a, b, ix, out, sub=False):
        f = lib().he355_sub if sub else lib().he355_add
        _check(f(self.h, L, size, n, a.ptr, b.ptr, ix, out.ptr))

    def multiply(self, L, n, a, b, ix, out):
        _check(lib().he355_multiply(self.h, L, n, a.ptr, b.ptr, ix, out.ptr))

    def bfv_multiply(self, L, n, a, b, ix, out):
        _check(lib().he355_bfv_multiply(self.h, L, n, a.ptr, b.ptr, ix, out.ptr))

    def multiply_relin(self, L, n, a, b, ix, out, rescale=False):
        _check(lib().he355_multiply_relin(self.h, L, n, a.ptr, b.ptr, ix, int(rescale), out.ptr))

    def relinearize(self, L, n, ct3, out):
        _check(lib().he355_relinearize(self.h, L, n, ct3.ptr, out.ptr))

    def multiply_plain(self, L, size, n, ct, pt, ix, out):
        _check(lib().he355_multiply_plain(self.h, L, size, n, ct.ptr, pt.ptr, ix, out.ptr))

    def add_plain(self, L, size, n, ct, pt, ix, out):
        _check(lib().he355_add_plain(self.h, L, size, n, ct.ptr, pt.ptr, ix, out.ptr))

    def mod_switch_drop(self, L, L_to, n_polys, inp, out):
        _check(lib().he355_mod_switch_drop(self.h, L, L_to, n_polys, inp.ptr, out.ptr))

    def bfv_mod_switch(self, L, L_to, size, n, inp, out):
        """BFV mod_switch_to: [n][size][L][N] -> [n][size][L_to][N] (L - L_to divide-and-round steps, one launch)"""
        _check(lib().he355_bfv_mod_switch(self.h, L, L_to, size, n, inp.ptr, out.ptr))

    def bfv_add_plain(self, L, size, n, ct, pt, ix, out, sub=False):
        """BFV add_plain / sub_plain: out = ct +- (Delta_L(pt), 0, ..); pt [.][N] coefficients mod t (bfv_encode's output)"""
        f = lib().he355_bfv_sub_plain if sub else lib().he355_bfv_add_plain
        _check(f(self.h, L, size, n, ct.ptr, pt.ptr, ix, out.ptr))

    def bfv_multiply_plain(self, L, size, n, ct, pt, ix, out):
        """BFV multiply_plain: every polynomial times the centred lift of pt, negacyclic; coefficient form in and out"""
        _check(lib().he355_bfv_multiply_plain(self.h, L, size, n, ct.ptr, pt.ptr, ix, out.ptr))

    def bfv_transform_to_ntt(self, L, size, n, inp, out):
        """BFV transform_to_ntt_inplace of ciphertexts [n][size][L][N]; out may be inp (in place).  The form of a slab is the caller's contract"""
        _check(lib().he355_bfv_transform_to_ntt(self.h, L, size, n, inp.ptr, out.ptr))

    def bfv_transform_from_ntt(self, L, size, n, inp, out):
        """BFV transform_from_ntt_inplace: NTT form -> coefficient form; out may be inp"""
        _check(lib().he355_bfv_transform_from_ntt(self.h, L, size, n, inp.ptr, out.ptr))

    def bfv_plain_to_ntt(self, L, n, pt, out):
        """pt [n][N] coefficients mod t (bfv_encode's output) -> out [n][L][N]: centred lift, NTT form under primes 0 .. L-1"""
        _check(lib().he355_bfv_plain_to_ntt(self.h, L, n, pt.ptr, out.ptr))

    def bfv_multiply_plain_ntt(self, L, size, n, ct, pt_ntt, ix, out):
        """BFV multiply_plain on NTT-form operands: every polynomial times the NTT-form plaintext (bfv_plain_to_ntt's output)"""
        _check(lib().he355_bfv_multiply_plain_ntt(self.h, L, size, n, ct.ptr, pt_ntt.ptr, ix, out.ptr))

    def bfv_multiply_plain_accumulate(self, L, size, rows, cols, inner, ct, ct_stride_i, ct_stride_k, pt_ntt, pt_stride_k, pt_stride_j, out):
        """out(i, j) = sum_k ct(i, k) (.) pt(k, j) over NTT-form operands, [rows * cols][size][L][N]: one launch, bit-identical to the loop"""
        _check(lib().he355_bfv_multiply_plain_accumulate(self.h, L, size, rows, cols, inner, ct.ptr, ct_stride_i, ct_stride_k, pt_ntt.ptr,
                                                         pt_stride_k, pt_stride_j, out.ptr))

    def bfv_multiply_monomial(self, L, size, n, inp, exponent, out):
        """out = inp * X^exponent in Z_q[X]/(X^N + 1) for every polynomial of [n][size][L][N]; exponent in [0, 2N), coefficient form"""
        _check(lib().he355_bfv_multiply_monomial(self.h, L, size, n, inp.ptr, exponent, out.ptr))

    def bfv_expand_galois_elts(self, count: int) -> list[int]:
        """the Galois elements bfv_expand needs for `count` children: N / 2^j + 1, j < ceil(log2 count) (host-side; no device needed)"""
        buf = (C.c_uint32 * 32)()
        d = lib().he355_bfv_expand_galois_elts(self.h, count, buf, 32)
        return [int(x) for x in buf[:d]]

    def bfv_expand(self, L, n, inp, count, out):
        """oblivious query expansion: inp [n][2][L][N] -> out [count][n][2][L][N], child k of query r at index k * n + r"""
        _check(lib().he355_bfv_expand(self.h, L, n, inp.ptr, count, out.ptr))

    def bfv_merge(self, L, n, count, inp, stride_k, stride_r, out):
        """the expansion's transpose: input k < count of result r < n at ciphertext k * stride_k + r * stride_r of inp -> out [n][2][L][N], whose
        plaintext holds 2^d times coefficient 2^d m of input k at coefficient k + 2^d m, d = ceil(log2 count); the Galois keys are those of
        bfv_expand_galois_elts(count)"""
        _check(lib().he355_bfv_merge(self.h, L, n, count, inp.ptr, stride_k, stride_r, out.ptr))

    def bfv_digit_count(self, L: int) -> tuple[int, list[int]]:
        """(D(L), [D_0 .. D_(L-1)]): how many plaintexts bfv_decompose cuts one residue polynomial into under each prime of level L, digits
        of bitlen(t) - 1 bits; a ciphertext of `size` polynomials becomes size * D(L) plaintexts.  (0, []) for a CKKS context or a bad level
        (host-side; no device needed)"""
        buf = (C.c_uint32 * 64)()
        total = int(lib().he355_bfv_digit_count(self.h, L, buf, 64))
        return total, [int(x) for x in buf[:L]] if total else []

    def bfv_decompose(self, L, size, n, ct, plain):
        """ct [n][size][L][N] coefficient form -> plain [n][F][N] mod t, F = size * D(L): polynomial k, prime i, digit g at k D(L) + off_i + g"""
        _check(lib().he355_bfv_decompose(self.h, L, size, n, ct.ptr, plain.ptr))

    def bfv_decompose_ntt(self, L, size, n, ct, L_out, plain_ntt):
        """ct [n][size][L][N] -> plain_ntt [n][F][L_out][N]: bfv_decompose followed by bfv_plain_to_ntt(L_out, n * F), fused; the pt operand of
        bfv_multiply_plain_accumulate with pt_stride_k = F, pt_stride_j = 1"""
        _check(lib().he355_bfv_decompose_ntt(self.h, L, size, n, ct.ptr, L_out, plain_ntt.ptr))

    def bfv_compose(self, L, size, n, plain, ct):
        """the inverse of bfv_decompose: plain [n][F][N] -> ct [n][size][L][N], canonical residues whatever the digits"""
        _check(lib().he355_bfv_compose(self.h, L, size, n, plain.ptr, ct.ptr))

    def bfv_gadget_count(self, L: int, digit_bits: int) -> tuple[int, list[int]]:
        """(E(L), [E_0 .. E_(L-1)]): the digits of width digit_bits (1..63) a residue under each prime of level L is cut into for the external
        product; an RGSW ciphertext has 2 E(L) rows.  (0, []) for a CKKS context, a bad level or a bad width (host-side; no device needed)"""
        buf = (C.c_uint32 * 64)()
        total = int(lib().he355_bfv_gadget_count(self.h, L, digit_bits, buf, 64))
        return total, [int(x) for x in buf[:L]] if total else []

    def bfv_gadget_decompose(self, L, digit_bits, size, n, ct, digits):
        """ct [n][size][L][N] coefficient form -> digits [n][size E][N]: the plain integer digits (no centred lift), polynomial k, prime i,
        digit g at k E(L) + off_i + g"""
        _check(lib().he355_bfv_gadget_decompose(self.h, L, digit_bits, size, n, ct.ptr, digits.ptr))

    def bfv_gadget_decompose_ntt(self, L, digit_bits, size, n, ct, digits_ntt):
        """ct [n][size][L][N] -> digits_ntt [n][size E][L][N]: bfv_gadget_decompose, then ntt_forward of every digit polynomial under every
        prime of the level (a digit not below q_j reduced first), fused"""
        _check(lib().he355_bfv_gadget_decompose_ntt(self.h, L, digit_bits, size, n, ct.ptr, digits_ntt.ptr))

    def bfv_rgsw_encrypt(self, L, digit_bits, n, plain, seed, first_index, rgsw):
        """plain [n][N] mod t -> rgsw [n][2E][2][L][N] NTT form: row f of RGSW r is encrypt_zero(seed, first_index + r 2E + f) cut to L primes
        plus lift(m) 2^(g v) in polynomial k under prime i (f = k E + off_i + g); needs set_public_key"""
        _check(lib().he355_bfv_rgsw_encrypt(self.h, L, digit_bits, n, plain.ptr, seed, first_index, rgsw.ptr))

    def bfv_external_product(self, L, digit_bits, n, inner, ct, ct_stride_r, ct_stride_k, rgsw, rg_stride_r, rg_stride_k, out):
        """out(r) = sum_kappa rgsw(r, kappa) [.] ct(r, kappa), [n][2][L][N], coefficient form in and out; ciphertext (r, kappa) at index
        r ct_stride_r + kappa ct_stride_k, RGSW (r, kappa) at r rg_stride_r + kappa rg_stride_k (rg_stride_r == 0: one selector row for all)"""
        _check(lib().he355_bfv_external_product(self.h, L, digit_bits, n, inner, ct.ptr, ct_stride_r, ct_stride_k, rgsw.ptr, rg_stride_r,
                                                rg_stride_k, out.ptr))

    def bfv_select(self, L, digit_bits, n, count, ct, ct_stride_r, ct_stride_k, rgsw, rg_stride_r, rg_stride_j, out):
        """the selection tree: out(r) [n][2][L][N] = the fold of result r's `count` leaves (leaf k at ciphertext r ct_stride_r + k ct_stride_k of ct)
        under its ceil(log2 count) RGSW bits (bit j at RGSW ciphertext r rg_stride_r + j rg_stride_j; rg_stride_r == 0: one set for all results),
        level by level node(2p) + RGSW(bit j) [.] (node(2p+1) - node(2p)): decrypts to leaf sum_j b_j 2^j, least significant bit first"""
        _check(lib().he355_bfv_select(self.h, L, digit_bits, n, count, ct.ptr, ct_stride_r, ct_stride_k, rgsw.ptr, rg_stride_r, rg_stride_j, out.ptr))

    def bfv_selector_encrypt(self, L, digit_bits, n, n_sel, first_slot, count, sel, seed, first_index, out):
        """sel [n][n_sel] mod t -> out [n][2][L][N], coefficient form: encrypt_zero(seed, first_index + r) cut to L primes plus, at coefficient
        first_slot + b E + off_i + g of polynomial 0 under prime i, lift(m) 2^(g v) (2^d)^(-1) mod q_i, d = ceil(log2 count): after
        bfv_expand(count) child first_slot + b E + f is row f (k = 0) of RGSW(m_(r,b)) before its transform; needs the public key"""
        _check(lib().he355_bfv_selector_encrypt(self.h, L, digit_bits, n, n_sel, first_slot, count, sel.ptr, seed, first_index, out.ptr))

    def bfv_rgsw_encrypt_secret(self, L, key_bits, seed, first_index, rgsw):
        """rgsw [2 E_key][2][L][N]: bfv_rgsw_encrypt of the secret key's coefficients mod t (the circular-security assumption); needs both keys"""
        _check(lib().he355_bfv_rgsw_encrypt_secret(self.h, L, key_bits, seed, first_index, rgsw.ptr))

    def bfv_rgsw_from_bfv(self, L, digit_bits, key_bits, n, n_sel, ct, ct_stride_r, ct_stride_k, key, rgsw):
        """rgsw [n][n_sel][2E][2][L][N] NTT form: row f of RGSW (r, b) is transform_to_ntt of the ciphertext at index
        r ct_stride_r + (b E + f) ct_stride_k of ct, row E + f its external product (key_bits) with key = RGSW(s), left in NTT form"""
        _check(lib().he355_bfv_rgsw_from_bfv(self.h, L, digit_bits, key_bits, n, n_sel, ct.ptr, ct_stride_r, ct_stride_k, key.ptr, rgsw.ptr))

    def bfv_bytes_per_plain(self) -> tuple[int, int]:
        """(Bmax, w): the most bytes one plaintext holds, floor(N w / 8), and the field width w = bitlen(t) - 1 of the byte codec; (0, 0)
        for a CKKS context (host-side; no device needed)"""
        w = C.c_uint32(0)
        return int(lib().he355_bfv_bytes_per_plain(self.h, C.byref(w))), int(w.value)

    @staticmethod
    def _at(buf, byte_offset):
        return C.c_void_p(buf.ptr.value + int(byte_offset))

    def bfv_unpack_bytes(self, n, buf, byte_offset, stride_bytes, bytes_per_plain, plain):
        """the B = bytes_per_plain bytes at byte_offset + j * stride_bytes of `buf` (any offset, any stride >= B), read as one little-endian
        integer -> plain [n][N]: coefficient e its bits [e w, e w + w)"""
        _check(lib().he355_bfv_unpack_bytes(self.h, n, self._at(buf, byte_offset), stride_bytes, bytes_per_plain, plain.ptr))

    def bfv_unpack_bytes_ntt(self, L_out, n, buf, byte_offset, stride_bytes, bytes_per_plain, plain_ntt):
        """bytes -> plain_ntt [n][L_out][N]: bfv_unpack_bytes followed by bfv_plain_to_ntt(L_out, n), fused; the pt operand of
        bfv_multiply_plain_accumulate"""
        _check(lib().he355_bfv_unpack_bytes_ntt(self.h, L_out, n, self._at(buf, byte_offset), stride_bytes, bytes_per_plain, plain_ntt.ptr))

    def bfv_pack_bytes(self, n, plain, bytes_per_plain, stride_bytes, buf, byte_offset=0):
        """the inverse of bfv_unpack_bytes: plain [n][N] (each word masked to w bits) -> ceil(B / 8) whole words per plaintext at
        byte_offset + j * stride_bytes of `buf` (both multiples of 8), the bytes past B in the last word zero"""
        _check(lib().he355_bfv_pack_bytes(self.h, n, plain.ptr, bytes_per_plain, stride_bytes, self._at(buf, byte_offset)))

    def bfv_reply_bytes(self, k0, k1) -> int:
        """bytes of one compressed reply, N (k0 + k1) / 8; 0 for a CKKS context or widths the chain refuses (host-side; no device needed)"""
        return int(lib().he355_bfv_reply_bytes(self.h, k0, k1))

    def bfv_reply_safe_bits(self):
        """(k0, k1, accepted): the widths bitlen(t) + 2 and bitlen(t) + 2 + log2 N under which every coefficient of a reply with at least 2
        bits of noise budget at L = 1 decrypts correctly, and whether this chain's first prime holds them (host-side; no device needed)"""
        k0, k1 = C.c_int32(0), C.c_int32(0)
        ok = lib().he355_bfv_reply_safe_bits(self.h, C.byref(k0), C.byref(k1))
        return int(k0.value), int(k1.value), bool(ok)

    def bfv_reply_compress(self, L, k0, k1, n, ct, buf, stride_bytes, byte_offset=0):
        """ct [n][2][L][N] coefficient form -> reply j at byte_offset + j * stride_bytes of `buf` (both multiples of 8): switched to L = 1,
        c0 cut to k0 bits and c1 to k1 bits per coefficient, bit-packed: bfv_reply_bytes(k0, k1) bytes each"""
        _check(lib().he355_bfv_reply_compress(self.h, L, k0, k1, n, ct.ptr, self._at(buf, byte_offset), stride_bytes))

    def bfv_reply_decrypt(self, k0, k1, n, buf, stride_bytes, plain, byte_offset=0, with_budget=False):
        """the replies at byte_offset + j * stride_bytes of `buf` -> plain [n][N] mod t (needs set_secret_key); with_budget: returns
        (budget, noise_bits), np.int32[n] each: max(0, k1 - noise_bits - 1) and the bit length of the largest rounding residue"""
        if not with_budget:
            _check(lib().he355_bfv_reply_decrypt(self.h, k0, k1, n, self._at(buf, byte_offset), stride_bytes, plain.ptr, None, None))
            return None
        out = DeviceBuffer(self, max(1, n))  # n budgets, then n noise_bits: int32 each, inside n uint64 words
        try:
            _check(lib().he355_bfv_reply_decrypt(self.h, k0, k1, n, self._at(buf, byte_offset), stride_bytes, plain.ptr, out.ptr, C.c_void_p(out.ptr.value + 4 * n)))
            v = out.download().view(np.int32)
        finally:
            out.free()
        return v[:n].copy(), v[n:2 * n].copy()

    def bfv_seeded_encrypt(self, L, n, plain, a_seed, noise_seed, first_index, c0):
        """(client) plain [n][N] mod t, or None for zeros -> c0 [n][L][N], coefficient form: Delta_L(m) - e - iNTT(a (.) s) with a the uniform
        half a_seed (PUBLIC) stands for and e drawn from noise_seed (SECRET, different); needs set_secret_key only"""
        _check(lib().he355_bfv_seeded_encrypt(self.h, L, n, plain.ptr if plain is not None else None, a_seed, noise_seed, first_index, c0.ptr))

    def bfv_seeded_selector_encrypt(self, L, digit_bits, n, n_sel, first_slot, count, sel, a_seed, noise_seed, first_index, c0):
        """(client) polynomial 0 of bfv_selector_encrypt over the seeded zero: c0 [n][L][N]"""
        _check(lib().he355_bfv_seeded_selector_encrypt(self.h, L, digit_bits, n, n_sel, first_slot, count, sel.ptr, a_seed, noise_seed, first_index, c0.ptr))

    def bfv_seeded_restore(self, L, ntt_form, n, c0, a_seed, first_index, out):
        """(server) c0 [n][L][N] -> out [n][2][L][N]: ntt_form 0: (c0, iNTT(a)), coefficient form; 1: (NTT(c0), a); needs no key"""
        _check(lib().he355_bfv_seeded_restore(self.h, L, ntt_form, n, c0.ptr, a_seed, first_index, out.ptr))

    def keygen_galois_seeded(self, elt, a_seed, noise_seed, b):
        """(client) the `b` halves [L_top][K][N] (NTT form) of the Galois key of `elt` whose `a` halves a_seed stands for, into the device
        buffer b; installs nothing"""
        _check(lib().he355_keygen_galois_seeded(self.h, elt, a_seed, noise_seed, b.ptr))

    def set_galois_key_seeded(self, elt, b_halves: np.ndarray, a_seed):
        """(server) set_galois_key of the key whose `b` halves are b_halves [L_top][K][N] (host) and whose `a` halves a_seed stands for"""
        k = np.ascontiguousarray(b_halves, dtype=np.uint64)
        assert k.size == self.L * self.K * self.N
        _check(lib().he355_set_galois_key_seeded(self.h, elt, k.ctypes.data_as(_u64p), a_seed))

    def bfv_noise_budget(self, L, size, n, ct, with_bits=False):
        """Decryptor::invariant_noise_budget of n ciphertexts [n][size][L][N] (size 2 or 3; needs set_secret_key): np.int32[n] bits of
        budget left at level L; with_bits: (budget, noise_bits), noise_bits the bit length of the invariant noise norm before the clamp"""
        out = DeviceBuffer(self, max(1, n))  # n budgets, then n noise_bits: int32 each, inside n uint64 words
        try:
            bits = C.c_void_p(out.ptr.value + 4 * n) if with_bits else None
            _check(lib().he355_bfv_noise_budget(self.h, L, size, n, ct.ptr, out.ptr, bits))
            v = out.download().view(np.int32)
        finally:
            out.free()
        return (v[:n].copy(), v[n:2 * n].copy()) if with_bits else v[:n].copy()

    def sum(self, L, size, n, inp, out):
        _check(lib().he355_sum(self.h, L, size, n, inp.ptr, out.ptr))

    def set_public_key(self, pk: np.ndarray):
        pk = np.ascontiguousarray(pk, dtype=np.uint64)
        _check(lib().he355_set_public_key(self.h, pk.ctypes.data))

    def set_secret_key(self, sk: np.ndarray):
        sk = np.ascontiguousarray(sk, dtype=np.uint64)
        _check(lib().he355_set_secret_key(self.h, sk.ctypes.data))

    def encrypt(self, n, plain, seed, first_index, out):
        _check(lib().he355_encrypt(self.h, n, plain.ptr, seed, first_index, out.ptr))

    def encrypt_zero(self, n, seed, first_index, out):
        _check(lib().he355_encrypt_zero(self.h, n, seed, first_index, out.ptr))

    def set_zero_stream(self, seed, first_index=0):
        _check(lib().he355_set_zero_stream(self.h, seed, first_index))

    def decrypt(self, L, size, n, ct, out):
        _check(lib().he355_decrypt(self.h, L, size, n, ct.ptr, out.ptr))

    def ckks_encode(self, n, values, count, scale, plain):
        _check(lib().he355_ckks_encode(self.h, n, values.ptr, count, scale, plain.ptr))

    def ckks_decode(self, L, n, plain, scale, out):
        _check(lib().he355_ckks_decode(self.h, L, n, plain.ptr, scale, out.ptr))

    def bfv_encode(self, n, values, count, plain):
        _check(lib().he355_bfv_encode(self.h, n, values.ptr, count, plain.ptr))

    def bfv_decode(self, n, plain, out):
        _check(lib().he355_bfv_decode(self.h, n, plain.ptr, out.ptr))

    @staticmethod
    def _ranges(ranges):
        flat = [int(v) for r in ranges for v in r]
        return (C.c_uint64 * len(flat))(*flat), len(flat) // 2

    def ckks_decode_slots(self, L, n, plain, scale, ranges, out):
        """only the slots of `ranges` = [(first, count), ...]: out is [n][sum of counts]"""
        arr, k = self._ranges(ranges)
        _check(lib().he355_ckks_decode_slots(self.h, L, n, plain.ptr, scale, arr, k, out.ptr))

    def bfv_decode_slots(self, n, plain, ranges, out):
        arr, k = self._ranges(ranges)
        _check(lib().he355_bfv_decode_slots(self.h, n, plain.ptr, arr, k, out.ptr))

    def relinearize_rescale(self, L, n, ct3, out):
        _check(lib().he355_relinearize_rescale(self.h, L, n, ct3.ptr, out.ptr))

    def multiply_accumulate(self, L, rows, cols, inner, a, a_stride_i, a_stride_k, b, b_stride_k, b_stride_j, out):
        _check(lib().he355_multiply_accumulate(self.h, L, rows, cols, inner, a.ptr, a_stride_i, a_stride_k, b.ptr, b_stride_k, b_stride_j, out.ptr))

    def bfv_multiply_relin_accumulate(self, L, rows, cols, inner, a, a_stride_i, a_stride_k, b, b_stride_k, b_stride_j, out):
        _check(lib().he355_bfv_multiply_relin_accumulate(self.h, L, rows, cols, inner, a.ptr, a_stride_i, a_stride_k, b.ptr, b_stride_k,
                                                         b_stride_j, out.ptr))

    def rescale(self, L, size, n, inp, out):
        _check(lib().he355_rescale(self.h, L, size, n, inp.ptr, out.ptr))

    def apply_galois(self, L, n, inp, elt, out):
        _check(lib().he355_apply_galois(self.h, L, n, inp.ptr, elt, out.ptr))

    def rotate(self, L, n, inp, step, out):
        _check(lib().he355_rotate(self.h, L, n, inp.ptr, step, out.ptr))

    def apply_galois_hoisted(self, L, n, inp, elts, out, ntt_form=True):
        """out [len(elts)][n][2][L][N]: block r = the hoisted Galois map of inp under elts[r] (1: the identity); one digit lift per chunk is
        shared by all elements, each of which needs its own Galois key.  Not bit-identical to apply_galois (include/he355.h)"""
        arr = (C.c_uint32 * max(1, len(elts)))(*[int(v) for v in elts])
        _check(lib().he355_apply_galois_hoisted(self.h, L, int(ntt_form), n, inp.ptr, arr, len(elts), out.ptr))

    def rotate_hoisted(self, L, n, inp, steps, out, ntt_form=True):
        """the same by steps (0: the identity); no NAF fallback"""
        arr = (C.c_int32 * max(1, len(steps)))(*[int(v) for v in steps])
        _check(lib().he355_rotate_hoisted(self.h, L, int(ntt_form), n, inp.ptr, arr, len(steps), out.ptr))

    def rotate_hoisted_plain_sum(self, L, n, inp, steps, plain, out):
        """out [n][2][L][N] = sum_r plain[r] (.) hoisted(inp, steps[r]); plain [len(steps)][L][N] NTT-form plaintexts; NTT-form ciphertexts"""
        arr = (C.c_int32 * max(1, len(steps)))(*[int(v) for v in steps])
        _check(lib().he355_rotate_hoisted_plain_sum(self.h, L, n, inp.ptr, arr, len(steps), plain.ptr, out.ptr))

    def rotate_hoisted_plain_sum_lazy(self, L, n, inp, steps, plain_qp, out):
        """out [n][2][L][N] = the same sum with ONE mod-down: the key products are accumulated in the extended basis; plain_qp
        [len(steps)][L + 1][N], row L under the special prime (plain_extend_special)"""
        arr = (C.c_int32 * max(1, len(steps)))(*steps)
        _check(lib().he355_rotate_hoisted_plain_sum_lazy(self.h, L, n, inp.ptr, arr, len(steps), plain_qp.ptr, out.ptr))

    def linear_transform_bsgs(self, L, n, inp, baby, giant, plain_qp, out, mask=None):
        """out [n][2][L][N] = sum_j rot_{giant[j]}(sum_i plain_qp[j][i] (.) rot_{baby[i]}(in)): plain_qp [len(giant)][len(baby)][L + 1][N],
        pre-rotated by -giant[j]; mask (optional): len(giant) x len(baby) flags, a zero drops the term"""
        b, g = (C.c_int32 * max(1, len(baby)))(*baby), (C.c_int32 * max(1, len(giant)))(*giant)
        m = None
        if mask is not None:
            flat = [int(bool(v)) for row in mask for v in row]
            m = (C.c_uint8 * max(1, len(flat)))(*flat)
        _check(lib().he355_linear_transform_bsgs(self.h, L, n, inp.ptr, b, len(baby), g, len(giant), plain_qp.ptr, m, out.ptr))

    def linear_transform_bsgs_scratch_bytes(self, L, n, n_baby) -> int:
        """an upper bound of the pool bytes linear_transform_bsgs takes for n ciphertexts at the context's batch chunk"""
        return int(lib().he355_linear_transform_bsgs_scratch_bytes(self.h, L, n, n_baby))

    def plain_extend_special(self, L, n, plain_ntt, plain_qp, mismatch=None):
        """plain_ntt [n][L][N] NTT form -> plain_qp [n][L + 1][N], row L under the special prime; mismatch (optional): one device word that
        receives the number of (coefficient, prime >= 1) pairs that disagree with prime 0"""
        _check(lib().he355_plain_extend_special(self.h, L, n, plain_ntt.ptr, plain_qp.ptr, mismatch.ptr if mismatch is not None else None))

    def hoist_stats(self, reset: bool = False) -> dict:
        """what the hoisted calls did (he355_hoist_stats): digit lifts, key products, permuted keys built, bytes those copies hold"""
        st = HoistStats()
        _check(lib().he355_hoist_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in HoistStats._fields_ if k != "reserved"}

    def combine_scalars(self, L, size, n, terms, scalars, out, const=None):
        """out [n][size][L][N] = sum_t scalars[t][i] * terms[t] + (polynomial 0: const[i]); terms: (buffer, level) pairs, a level >= L read
        with its own stride; scalars: len(terms) rows of L canonical residues; const: L residues or None"""
        tt = (Term * max(1, len(terms)))(*[Term(getattr(b.ptr, "value", b.ptr), int(lv), 0) for b, lv in terms])
        flat = [int(v) for row in scalars for v in row]
        sc = (C.c_uint64 * max(1, len(flat)))(*flat)
        cc = (C.c_uint64 * L)(*[int(v) for v in const]) if const is not None else None
        _check(lib().he355_combine_scalars(self.h, L, size, n, tt, len(terms), sc, cc, out.ptr))

    def ckks_scalar_residues(self, L, v) -> list:
        """the residues of the integer nearest v (ties to even) under the first L primes"""
        out = (C.c_uint64 * max(1, L))()
        _check(lib().he355_ckks_scalar_residues(self.h, L, float(v), out))
        return [int(x) for x in out[:L]]

    def ckks_eval_poly_plan(self, L, coeffs, log_baby, in_scale, out_scale, n=1) -> dict:
        """what ckks_eval_poly would do (he355_poly_plan_t): depth, L_out, counts per chunk, the powers computed, min_scalar_bits, pool_bytes"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        pl = PolyPlan()
        _check(lib().he355_ckks_eval_poly_plan(self.h, L, cs, len(coeffs), log_baby, in_scale, out_scale, n, C.byref(pl)))
        d = {k: getattr(pl, k) for k, _ in PolyPlan._fields_ if k not in ("reserved", "power_mask")}
        d["powers_computed"] = [k for k in range(1024) if (pl.power_mask[k // 64] >> (k % 64)) & 1]
        return d

    def ckks_eval_poly(self, L, n, inp, coeffs, log_baby, in_scale, out_scale, out):
        """out [n][2][L - depth][N] = sum_k coeffs[k] in^k at the nominal scale out_scale; inp [n][2][L][N] at in_scale"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        _check(lib().he355_ckks_eval_poly(self.h, L, n, inp.ptr, cs, len(coeffs), log_baby, in_scale, out_scale, out.ptr))

    def poly_stats(self, reset: bool = False) -> dict:
        """what combine_scalars and ckks_eval_poly ran (he355_poly_stats)"""
        st = PolyStats()
        _check(lib().he355_poly_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in PolyStats._fields_ if k != "reserved"}

    # ---- complex slots ----
    def ckks_encode_complex(self, n, values, count, scale, plain):
        """values [n][count][2] doubles (re, im) -> plain [n][L_top][N]; the conjugate slots hold conj(v)"""
        _check(lib().he355_ckks_encode_complex(self.h, n, values.ptr, count, scale, plain.ptr))

    def ckks_decode_complex(self, L, n, plain, scale, out):
        """out [n][N/2][2]: (re, im) of every slot"""
        _check(lib().he355_ckks_decode_complex(self.h, L, n, plain.ptr, scale, out.ptr))

    def ckks_decode_complex_slots(self, L, n, plain, scale, ranges, out):
        """only the slots of `ranges` = [(first, count), ...]: out is [n][sum of counts][2]"""
        arr, k = self._ranges(ranges)
        _check(lib().he355_ckks_decode_complex_slots(self.h, L, n, plain.ptr, scale, arr, k, out.ptr))

    def ckks_complex_unit(self, L) -> list:
        """u_i = NTT_{q_i}(X^(N/4) + X^(3N/4))[0] for the first L primes: u_i^2 = -2 (mod q_i)"""
        out = (C.c_uint64 * max(1, L))()
        _check(lib().he355_ckks_complex_unit(self.h, L, out))
        return [int(x) for x in out[:L]]

    def ckks_complex_scalar_residues(self, L, v_re, v_im) -> list:
        """[[(A + B u_i) % q_i], [(A - B u_i) % q_i]] with A = round(v_re), B = round(v_im / sqrt(2))"""
        out = (C.c_uint64 * max(1, 2 * L))()
        _check(lib().he355_ckks_complex_scalar_residues(self.h, L, float(v_re), float(v_im), out))
        return [[int(x) for x in out[:L]], [int(x) for x in out[L:2 * L]]]

    def combine_scalars_complex(self, L, size, n, terms, scalars, out, const=None):
        """combine_scalars with two residues per (term, prime): scalars[t] = [L residues where bit (log2 N - 2) of the NTT index is 0,
        L residues where it is 1]; const: such a pair or None"""
        tt = (Term * max(1, len(terms)))(*[Term(getattr(b.ptr, "value", b.ptr), int(lv), 0) for b, lv in terms])
        flat = [int(v) for pair in scalars for row in pair for v in row]
        sc = (C.c_uint64 * max(1, len(flat)))(*flat)
        cc = (C.c_uint64 * (2 * L))(*[int(v) for row in const for v in row]) if const is not None else None
        _check(lib().he355_combine_scalars_complex(self.h, L, size, n, tt, len(terms), sc, cc, out.ptr))

    @staticmethod
    def _parts(coeffs):
        re = (C.c_double * max(1, len(coeffs)))(*[complex(c).real for c in coeffs])
        im = (C.c_double * max(1, len(coeffs)))(*[complex(c).imag for c in coeffs])
        return re, im

    def ckks_eval_poly_complex_plan(self, L, coeffs, log_baby, in_scale, out_scale, n=1) -> dict:
        """ckks_eval_poly_plan for complex coefficients (Python complex numbers)"""
        re, im = self._parts(coeffs)
        pl = PolyPlan()
        _check(lib().he355_ckks_eval_poly_complex_plan(self.h, L, re, im, len(coeffs), log_baby, in_scale, out_scale, n, C.byref(pl)))
        d = {k: getattr(pl, k) for k, _ in PolyPlan._fields_ if k not in ("reserved", "power_mask")}
        d["powers_computed"] = [k for k in range(1024) if (pl.power_mask[k // 64] >> (k % 64)) & 1]
        return d

    def ckks_eval_poly_complex(self, L, n, inp, coeffs, log_baby, in_scale, out_scale, out):
        """ckks_eval_poly for complex coefficients (Python complex numbers): every leaf is one combine_scalars_complex"""
        re, im = self._parts(coeffs)
        _check(lib().he355_ckks_eval_poly_complex(self.h, L, n, inp.ptr, re, im, len(coeffs), log_baby, in_scale, out_scale, out.ptr))

    def ckks_mod_raise(self, L_in, L_to, size, n, inp, out):
        """out [n][size][L_to][N] = the residue under q_0 of inp [n][size][L_in][N] (row 0 of every polynomial; the rest is ignored), read as
        centred integers and re-expressed under q_0 .. q_{L_to - 1}, NTT form in and out (he355_ckks_mod_raise)"""
        _check(lib().he355_ckks_mod_raise(self.h, L_in, L_to, size, n, inp.ptr, out.ptr))

    def ckks_lift_centred(self, L_to, n_polys, coeff, out):
        """out [n_polys][L_to][N] = the coefficients coeff [n_polys][N] (canonical under q_0), centred, mod q_j in row j; coefficient form"""
        _check(lib().he355_ckks_lift_centred(self.h, L_to, n_polys, coeff.ptr, out.ptr))

    def raise_stats(self, reset: bool = False) -> dict:
        """what ckks_mod_raise and ckks_lift_centred ran (he355_raise_stats)"""
        st = RaiseStats()
        _check(lib().he355_raise_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in RaiseStats._fields_ if k != "reserved"}

    # ---- EvalMod: the fused combine-and-rescale step, Chebyshev evaluation, double angles ----
    def combine_scalars_rescale(self, L, size, n, terms, scalars, out, const=None):
        """out [n][size][L - 1][N] = rescale(combine_scalars(...)) bit for bit, without the combined slab; arguments as combine_scalars"""
        tt = (Term * max(1, len(terms)))(*[Term(getattr(b.ptr, "value", b.ptr), int(lv), 0) for b, lv in terms])
        flat = [int(v) for row in scalars for v in row]
        sc = (C.c_uint64 * max(1, len(flat)))(*flat)
        cc = (C.c_uint64 * max(1, L))(*[int(v) for v in const]) if const is not None else None
        _check(lib().he355_combine_scalars_rescale(self.h, L, size, n, tt, len(terms), sc, cc, out.ptr))

    @staticmethod
    def _plan_dict(pl):
        d = {k: getattr(pl, k) for k, _ in PolyPlan._fields_ if k not in ("reserved", "power_mask")}
        d["powers_computed"] = [k for k in range(1024) if (pl.power_mask[k // 64] >> (k % 64)) & 1]
        d["double_angles"] = int(pl.reserved[0])
        return d

    def ckks_eval_chebyshev_plan(self, L, coeffs, log_baby, in_scale, out_scale, n=1) -> dict:
        """what ckks_eval_chebyshev would do (he355_poly_plan_t; `rescales` counts the fused steps)"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        pl = PolyPlan()
        _check(lib().he355_ckks_eval_chebyshev_plan(self.h, L, cs, len(coeffs), log_baby, in_scale, out_scale, n, C.byref(pl)))
        return self._plan_dict(pl)

    def ckks_eval_chebyshev(self, L, n, inp, coeffs, log_baby, in_scale, out_scale, out):
        """out [n][2][L - depth][N] = sum_k coeffs[k] T_k(in) at the nominal scale out_scale; inp [n][2][L][N] at in_scale, slots in [-1, 1]"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        _check(lib().he355_ckks_eval_chebyshev(self.h, L, n, inp.ptr, cs, len(coeffs), log_baby, in_scale, out_scale, out.ptr))

    def ckks_eval_mod_plan(self, L, coeffs, log_baby, in_scale, out_scale, double_angles, n=1) -> dict:
        """what ckks_eval_mod would do; out_scale: the scale the output carries (s_r)"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        pl = PolyPlan()
        _check(lib().he355_ckks_eval_mod_plan(self.h, L, cs, len(coeffs), log_baby, in_scale, out_scale, double_angles, n, C.byref(pl)))
        return self._plan_dict(pl)

    def ckks_eval_mod(self, L, n, inp, coeffs, log_baby, in_scale, out_scale, double_angles, out):
        """the Chebyshev polynomial, then double_angles steps y <- 2 y^2 - 1; out [n][2][L - depth - double_angles][N]"""
        cs = (C.c_double * max(1, len(coeffs)))(*[float(c) for c in coeffs])
        _check(lib().he355_ckks_eval_mod(self.h, L, n, inp.ptr, cs, len(coeffs), log_baby, in_scale, out_scale, double_angles, out.ptr))

    def cheb_stats(self, reset: bool = False) -> dict:
        """what combine_scalars_rescale, ckks_eval_chebyshev and ckks_eval_mod ran (he355_cheb_stats)"""
        st = ChebStats()
        _check(lib().he355_cheb_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in ChebStats._fields_}

    def hoist_release_keys(self):
        _check(lib().he355_hoist_release_keys(self.h))

    def rotate_each(self, L, n, inp, steps, out):
        arr = (C.c_int32 * n)(*[int(v) for v in steps])
        _check(lib().he355_rotate_each(self.h, L, n, inp.ptr, arr, out.ptr))

    def set_latency_max(self, n=None):
        """largest batch whose key switches take the latency shape; None: the library's rule (batch * N <= 2^17, at most 12)"""
        _check(lib().he355_set_latency_max(self.h, 2 ** 64 - 1 if n is None else n))

    def set_lds_max(self, n=None):
        """largest batch whose key switches take the ring-in-LDS shape (N <= 8192); None: the library's rule; 0: never"""
        _check(lib().he355_set_lds_max(self.h, 2 ** 64 - 1 if n is None else n))

    def set_level_walk(self, on: bool):
        _check(lib().he355_set_level_walk(self.h, int(on)))

    def mem_info(self):
        """(free, total) bytes of the context's device"""
        f, t = C.c_uint64(), C.c_uint64()
        _check(lib().he355_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def alloc_stats(self) -> dict:
        """raw hipMalloc / hipFree calls and pool hits / misses of this context since device_init"""
        st = AllocStats()
        _check(lib().he355_alloc_stats(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in AllocStats._fields_}

    def path_stats(self, reset: bool = False) -> dict:
        """which key-switch shape / schedule ran (he355_path_stats): counts of kernel sequences since device_init or the last reset"""
        st = PathStats()
        _check(lib().he355_path_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in PathStats._fields_ if k != "reserved"}

    def bfv_route_stats(self, reset: bool = False) -> dict:
        """which route the BFV PIR calls took (he355_bfv_route_stats): counts of cuts, passes and calls since device_init or the last reset"""
        st = BfvRouteStats()
        _check(lib().he355_bfv_route_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in BfvRouteStats._fields_ if k != "reserved"}

    def bfv_multiply_stats(self, reset: bool = False) -> dict:
        """which route the BEHZ multiplies took (he355_bfv_multiply_stats): counts of calls, chunks and launches by kind since device_init or
        the last reset, and `lds_limit`, the dynamic LDS in bytes the device grants one block of the fused column kernels (not a counter)"""
        st = BfvMultiplyStats()
        _check(lib().he355_bfv_multiply_stats(self.h, C.byref(st), int(reset)))
        return {k: int(getattr(st, k)) for k, _ in BfvMultiplyStats._fields_ if k != "reserved"}

    def pool_trim(self) -> int:
        b = C.c_uint64()
        _check(lib().he355_pool_trim(self.h, C.byref(b)))
        return int(b.value)

    def rotate_sum(self, L, n, inp, steps, out):
        """out = inp + sum_j rotate(inp, steps[j]) with shared NAF prefixes; returns the Galois key switches issued per ciphertext"""
        arr = (C.c_int32 * len(steps))(*[int(v) for v in steps])
        ks = C.c_uint64(0)
        _check(lib().he355_rotate_sum(self.h, L, n, inp.ptr, arr, len(steps), out.ptr, C.byref(ks)))
        return int(ks.value)

    def rotate_add(self, L, n, inp, step, addend, out):
        _check(lib().he355_rotate_add(self.h, L, n, inp.ptr, step, addend.ptr, out.ptr))

    def accumulate(self, L, n, inout, count, tmp):
        _check(lib().he355_accumulate(self.h, L, n, inout.ptr, count, tmp.ptr))

    def ntt(self, buf, n_polys, prime_of, inverse=False):
        pm = (C.c_uint8 * len(prime_of))(*prime_of)
        f = lib().he355_ntt_inverse if inverse else lib().he355_ntt_forward
        _check(f(self.h, buf.ptr, n_polys, pm, len(prime_of)))

    # -- timing on the kernels' stream -----------------------------------------------------------
    def timer_begin(self):
        _check(lib().he355_timer_begin(self.h))

    def probe_dominant_kernel(self):
        """(total ms, launches, ops) of the k_k3<fp64> launches inside the last timer_begin/timer_end region."""
        ms, n, ops = C.c_float(), C.c_uint64(), C.c_uint64()
        _check(lib().he355_probe_dominant_kernel(self.h, C.byref(ms), C.byref(n), C.byref(ops)))
        return float(ms.value), int(n.value), int(ops.value)

    def clock_probe_begin(self, duration_us: int):
        """one wave on its own stream samples shader cycles against the 100 MHz counter for `duration_us` while what is queued next runs"""
        _check(lib().he355_clock_probe_begin(self.h, int(duration_us)))

    def clock_probe_end(self):
        """(MHz held, seconds covered) of the probe started by clock_probe_begin"""
        mhz, sec = C.c_double(0), C.c_double(0)
        _check(lib().he355_clock_probe_end(self.h, C.byref(mhz), C.byref(sec)))
        return mhz.value, sec.value

    def timer_end(self) -> float:
        ms = C.c_float()
        _check(lib().he355_timer_end(self.h, C.byref(ms)))
        return float(ms.value)


def eval_mod_coeffs(K: int, r: int, degree: int) -> list:
    """The Chebyshev coefficients he355_ckks_eval_mod takes: the interpolant of cos((2 pi / 2^r) (K u - 1/4)) on [-1, 1] at degree + 1
    Chebyshev points (numpy's chebinterpolate).  With in_scale = q_0 K and r double angles the call computes sin(2 pi t / q_0)."""
    w = 2.0 * np.pi / float(1 << r)
    return [float(c) for c in np.polynomial.chebyshev.chebinterpolate(lambda u: np.cos(w * (K * u - 0.25)), degree)]


def process_alloc_stats() -> dict:
    """totals over every context of this process (the benchmark objects behind API-Bridge handles own theirs)"""
    st = AllocStats()
    _check(lib().he355_alloc_stats(None, C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in AllocStats._fields_}


def device_count() -> int:
    n = C.c_int(0)
    lib().he355_device_count(C.byref(n))
    return int(n.value)
