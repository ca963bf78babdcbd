// cheb_args.h -- the argument checks of he355_combine_scalars_rescale and the host plans of he355_ckks_eval_chebyshev and
// he355_ckks_eval_mod, made ONCE per call in the style of poly_args.h, whose checks and planner they are under their own names: the C ABI
// function (ckks_eval_mod.inc) runs them before it asks for a device -- a refusal is HE355_E_INVALID_ARGS whether a device exists or not.
// Host-only on purpose: no HIP header, so tests/ckks_eval_mod_args_main.cpp runs every check at its edges under the sanitizers.
// The definitions are written out in include/he355.h; tests/ckks_eval_mod_ref.py restates them on the oracle.
#pragma once
#include "poly_args.h"

namespace he355 {

// ---- he355_combine_scalars_rescale -----------------------------------------------------------------------------------------------------
// True: n == 0, or no term and no constant -- the call touches nothing.  he355_combine_scalars' refusals, plus a BFV context, L < 2 and an
// overlap of the [n][size][L - 1][N] output with a term.
inline bool plan_combine_scalars_rescale(const Params &p, int L, int size, u64 n, const he355_term *terms, u64 n_terms, const u64 *scalars, const u64 *cst, const u64 *out)
{
    const std::string w("he355_combine_scalars_rescale");
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(w + ": the rescale is a CKKS operation");
    check_level(p, w, L);
    if (L < 2) throw std::invalid_argument(w + ": cannot rescale at the last level (L must be at least 2)");
    return plan_combine_scalars(p, w, L, size, n, terms, n_terms, scalars, cst, out, 1, L - 1);
}

// ---- he355_ckks_eval_chebyshev, he355_ckks_eval_mod ---------------------------------------------------------------------------------------
inline PolyPlan plan_eval_chebyshev(const Params &p, const char *what, int L, u64 n, const u64 *in, const double *coeffs, u64 n_coeffs, int log_baby, double in_scale,
                                    double out_scale, const u64 *out, bool check_ptrs, u64 chunk)
{
    return plan_eval_poly(p, what, L, n, in, coeffs, n_coeffs, log_baby, in_scale, out_scale, out, check_ptrs, chunk, nullptr, false, kBasisChebyshev, 0);
}
inline PolyPlan plan_eval_mod(const Params &p, const char *what, int L, u64 n, const u64 *in, const double *coeffs, u64 n_coeffs, int log_baby, double in_scale,
                              double out_scale, int double_angles, const u64 *out, bool check_ptrs, u64 chunk)
{
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(std::string(what) + ": polynomial evaluation is a CKKS operation");
    if (double_angles < 0 || double_angles > 8) throw std::invalid_argument(std::string(what) + ": double_angles must be 0..8");
    return plan_eval_poly(p, what, L, n, in, coeffs, n_coeffs, log_baby, in_scale, out_scale, out, check_ptrs, chunk, nullptr, false, kBasisChebyshev, double_angles);
}

} // namespace he355
