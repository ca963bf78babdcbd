// raise_args.h -- the argument checks of he355_ckks_mod_raise and he355_ckks_lift_centred, made ONCE per call in the style of poly_args.h:
// the C ABI function (ckks_poly_raise.inc) runs them before it asks for a device -- a refusal is HE355_E_INVALID_ARGS whether a device
// exists or not -- and then only launches.  Host-only on purpose: no HIP header, so tests/ckks_mod_raise_args_main.cpp runs every check at its edges
// under the sanitizers.  The definition of the raise is written out in include/he355.h; tests/ckks_mod_raise_ref.py restates it on the oracle.
#pragma once
#include <string>

#include "../../include/he355.h"
#include "bfv_pir_args.h"
#include "raise_core.h"

namespace he355 {

// the kernels move two words at a time (16-byte accesses); every row starts a multiple of N words behind its slab, so the slab's own
// address decides
inline void raise_check_aligned(const std::string &w, const void *p, const char *name)
{
    if ((unsigned long long)p & 15) throw std::invalid_argument(w + ": `" + name + "` must be 16-byte aligned");
}
inline void raise_check_scheme(const Params &p, const std::string &w)
{
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(w + ": the modulus raise is a CKKS operation (a BFV context has no level to raise to)");
}

// d_in [n][size][L_in][N] (row 0 of every polynomial is read; the ignored rows count as part of it) -> d_out [n][size][L_to][N].
// True: n == 0 -- the call touches nothing.
inline bool plan_mod_raise(const Params &p, int L_in, int L_to, int size, u64 n, const u64 *in, const u64 *out)
{
    const std::string w("he355_ckks_mod_raise");
    raise_check_scheme(p, w);
    if (L_in < 1 || (size_t)L_in > p.Ltop) throw std::invalid_argument(w + ": input level out of range");
    if (L_to < 1 || (size_t)L_to > p.Ltop) throw std::invalid_argument(w + ": target level out of range");
    if (size < 1 || size > 3) throw std::invalid_argument(w + ": ciphertext size must be 1..3");
    // every slab in words, formed in 128 bits: 2^60 words (2^63 bytes) is the most one may span
    const u128 cap = (u128)1 << 60, in_w = (u128)n * (u128)size * (u128)L_in * p.N, out_w = (u128)n * (u128)size * (u128)L_to * p.N;
    if (n > cap || in_w > cap || out_w > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    if (n == 0) return true;
    if (!in || !out) throw std::invalid_argument(w + ": null ciphertexts");
    if (word_range(w, out, (u64)out_w).overlaps(word_range(w, in, (u64)in_w))) throw std::invalid_argument(w + ": `d_out` overlaps `d_in`");
    raise_check_aligned(w, in, "d_in");
    raise_check_aligned(w, out, "d_out");
    return false;
}

// d_coeff [n_polys][N] -> d_out [n_polys][L_to][N].  True: n_polys == 0.
inline bool plan_lift_centred(const Params &p, int L_to, u64 n_polys, const u64 *coeff, const u64 *out)
{
    const std::string w("he355_ckks_lift_centred");
    raise_check_scheme(p, w);
    if (L_to < 1 || (size_t)L_to > p.Ltop) throw std::invalid_argument(w + ": target level out of range");
    const u128 cap = (u128)1 << 60, in_w = (u128)n_polys * p.N, out_w = (u128)n_polys * (u128)L_to * p.N;
    if (n_polys > cap || in_w > cap || out_w > cap) throw std::invalid_argument(w + ": the polynomials span more than 2^60 words");
    if (n_polys == 0) return true;
    if (!coeff || !out) throw std::invalid_argument(w + ": null polynomials");
    if (word_range(w, out, (u64)out_w).overlaps(word_range(w, coeff, (u64)in_w))) throw std::invalid_argument(w + ": `d_out` overlaps `d_coeff`");
    raise_check_aligned(w, coeff, "d_coeff");
    raise_check_aligned(w, out, "d_out");
    return false;
}

} // namespace he355
