// cplx_core.h -- the per-coefficient arithmetic of the complex scalar combination (he355_combine_scalars_complex; k_scalar_combine_cplx in
// he355_kernels_cplx.hip) and the residue rule of he355_ckks_complex_scalar_residues, host-compilable: tests/csim/sim_cplx.cpp runs the
// same text on the CPU and tests/test_ckks_complex_core_cpu.py holds it to Python integers.
//
// The encoders place slot j at zeta^(3^j), where X^(N/2) is i (-1)^j and not i.  J(X) = X^(N/4) + X^(3N/4) decodes to sqrt(2) i in EVERY
// slot, and in NTT form it takes two values per prime: u = NTT_q(J)[0] where bit (log2 N - 2) of the NTT index is 0, q - u where it is 1
// (u^2 = -2 mod q).  A complex constant at weight W is the integer polynomial A + B J, A = rint(Re W), B = rint(Im W / sqrt 2): ONE of two
// residues per (term, prime), A +- B u, picked by that bit.  The combination is poly_core.h's with the scalar and the opening constant
// picked per element; any pair of canonical residues is allowed.
#pragma once
#include "poly_core.h"

namespace he355 {

// s(e): which of the two residues NTT index e takes
HE_HD u32 cplx_half(u64 e, int logN) { return (u32)(e >> (logN - 2)) & 1u; }

// One element of the combination at half s: term k reads x[k * sx] and a[k * sa + s * sh]; cst the constant's residue of that half (0: none)
HE_HD u64 cplx_combine_sum(const u64 *x, u64 sx, const u64 *a, u64 sa, u64 sh, u32 s, u64 terms, u64 cst, u64 run, const ModU64 &m)
{
    return poly_combine_sum(x, sx, a + (u64)s * sh, sa, terms, cst, run, m);
}

// he355_ckks_complex_scalar_residues: A = the integer nearest v_re, B = the integer nearest v_im / sqrt(2.0) (an IEEE division), both by
// poly_scalar_integer's rule.  False: a part is not finite or not below 2^126 in magnitude.
inline bool cplx_scalar_integers(double v_re, double v_im, u128 &mag_a, bool &neg_a, u128 &mag_b, bool &neg_b)
{
    return poly_scalar_integer(v_re, mag_a, neg_a) && poly_scalar_integer(v_im / std::sqrt(2.0), mag_b, neg_b);
}
// (A + B u) mod q and (A - B u) mod q, canonical; u < q
inline void cplx_scalar_pair(u128 mag_a, bool neg_a, u128 mag_b, bool neg_b, u64 u, u64 q, u64 &plus, u64 &minus)
{
    const u64 a = poly_scalar_residue(mag_a, neg_a, q);
    const u64 bu = (u64)((u128)poly_scalar_residue(mag_b, neg_b, q) * u % q);
    plus = (u64)(((u128)a + bu) % q);
    minus = (u64)(((u128)a + (bu ? q - bu : 0)) % q);
}

} // namespace he355
