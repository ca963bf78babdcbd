// cplx_args.h -- the argument checks of the complex-slot calls that are theirs alone: he355_ckks_complex_unit,
// he355_ckks_complex_scalar_residues, he355_ckks_encode_complex and he355_ckks_decode_complex(_slots).  The checks of
// he355_combine_scalars_complex and he355_ckks_eval_poly_complex are he355_combine_scalars' and he355_ckks_eval_poly's under the new
// names (poly_args.h, which includes this file for the residue pairs of its planner).  The C ABI functions (ckks_complex.inc) run them
// before they ask for a device: a refusal is HE355_E_INVALID_ARGS whether a device exists or not.
// Host-only on purpose: no HIP header, so tests/ckks_complex_args_main.cpp runs every check at its edges under the sanitizers.
#pragma once
#include <string>

#include "../../include/he355.h"
#include "bfv_pir_args.h"
#include "client/ckks_codec.h"
#include "cplx_core.h"

namespace he355 {

// u = NTT_q(J)[0], J = X^(N/4) + X^(3N/4): NTT index 0 evaluates at the table's root psi, so u = psi^(N/4) + psi^(3N/4); u^2 = -2 mod q
inline u64 cplx_unit(const PrimeTables &pt, size_t N)
{
    const u64 w = Params::powmod(pt.root, N / 4, pt.q), w3 = (u64)((u128)w * w % pt.q * w % pt.q);
    return (u64)(((u128)w + w3) % pt.q);
}
// ---- he355_ckks_complex_unit ---------------------------------------------------------------------------------------------------------
inline void cplx_units(const Params &p, const std::string &w, int L, u64 *out)
{
    check_level(p, w, L);
    if (!out) throw std::invalid_argument(w + ": null output");
    for (int i = 0; i < L; ++i) out[i] = cplx_unit(p.primes[i], p.N);
}
// ---- he355_ckks_complex_scalar_residues: out [2][L] = (A + B u_i, A - B u_i) mod q_i -----------------------------------------------------
// mags (optional): |A| and |B|, for the planner's min_scalar_bits
inline void cplx_scalar_residues(const Params &p, const std::string &w, int L, double v_re, double v_im, u64 *out, u128 *mags = nullptr)
{
    check_level(p, w, L);
    if (!out) throw std::invalid_argument(w + ": null output");
    u128 ma, mb;
    bool na, nb;
    if (!cplx_scalar_integers(v_re, v_im, ma, na, mb, nb)) throw std::invalid_argument(w + ": a part of the scalar is not finite or not below 2^126 in magnitude");
    for (int i = 0; i < L; ++i) cplx_scalar_pair(ma, na, mb, nb, cplx_unit(p.primes[i], p.N), p.primes[i].q, out[i], out[(size_t)L + (size_t)i]);
    if (mags) { mags[0] = ma; mags[1] = mb; }
}
// ---- the complex codec.  True: n == 0, the call touches nothing ----------------------------------------------------------------------------
inline bool plan_encode_complex(const Params &p, u64 n, const double *values, u64 count, double scale, const u64 *plain)
{
    const std::string w("he355_ckks_encode_complex");
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(w + ": needs a CKKS context");
    if (count > p.N / 2) throw std::invalid_argument(w + ": Not enough slots available to create packed plaintext");
    if (!std::isfinite(scale) || scale <= 0) throw std::invalid_argument(w + ": the scale must be finite and positive");
    const u128 cap = (u128)1 << 60;
    if (n > cap || (u128)n * p.Ltop * p.N > cap) throw std::invalid_argument(w + ": the plaintexts span more than 2^60 words");
    if (n == 0) return true;
    if (!plain || (count && !values)) throw std::invalid_argument(w + ": null pointer");
    word_range(w, plain, n * p.Ltop * p.N);
    byte_range(w, values, 16 * n * count);
    return false;
}
// sr: the checked ranges (ranges == null: every slot).  True: nothing to write.
inline bool plan_decode_complex(const Params &p, const char *what, int L, u64 n, const u64 *plain, double scale, const u64 *ranges, u64 n_ranges, bool slots,
                                const double *out, SlotRanges &sr)
{
    const std::string w(what);
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(w + ": needs a CKKS context");
    check_level(p, w, L);
    if (L > 16) throw std::invalid_argument(w + ": decoding supports up to 16 data primes");
    if (!std::isfinite(scale) || scale <= 0) throw std::invalid_argument(w + ": the scale must be finite and positive");
    if (slots && !ranges) throw std::invalid_argument(w + ": null ranges");
    try {
        sr = slot_ranges(ranges, n_ranges, p.N / 2);
    } catch (const std::invalid_argument &e) {
        throw std::invalid_argument(w + ": " + e.what());
    }
    const u128 cap = (u128)1 << 60;
    if (n > cap || (u128)n * (u128)L * p.N > cap) throw std::invalid_argument(w + ": the plaintexts span more than 2^60 words");
    if (n == 0 || sr.total == 0) return true;
    if (!plain || !out) throw std::invalid_argument(w + ": null pointer");
    word_range(w, plain, n * (u64)L * p.N);
    byte_range(w, out, 16 * n * sr.total);
    return false;
}

} // namespace he355
