// poly_core.h -- the per-coefficient arithmetic of the scalar combination (he355_combine_scalars; k_scalar_combine in
// he355_kernels_poly.hip) and the scalar-residue rule of he355_ckks_scalar_residues, host-compilable: tests/csim/sim_poly.cpp runs the
// same text on the CPU and tests/test_ckks_eval_poly_core_cpu.py holds it to Python integers.
//
//   out = (sum_t a_t x_t + c) mod q over canonical residues, a constant polynomial being ONE residue per prime in the NTT domain.  The
//   products are added unreduced into one 128-bit sum under the run rule of bfv_mac_core.h as k_bsgs_inner walks it (bsgs_run_full): the
//   constant (at most q - 1, no more than one product) opens the first run as a folded residue opens every later one, so a run takes
//   run - 1 products behind it.  The result is the canonical residue of the exact integer sum wherever the runs are cut.
#pragma once
#include <cmath>

#include "bsgs_core.h"

namespace he355 {

// one run length for all primes of a launch (bsgs_run: the shortest; 256 under a 60-bit prime)
inline u64 poly_run(const u64 *q, int n_primes) { return bsgs_run(q, n_primes); }

// One element of the combination: term k reads x[k * sx] and a[k * sa]; cst is the constant's residue (0: none)
HE_HD u64 poly_combine_sum(const u64 *x, u64 sx, const u64 *a, u64 sa, u64 terms, u64 cst, u64 run, const ModU64 &m)
{
    u128 acc = cst;
    u64 left = run - 1;
    for (u64 k = 0; k < terms; ++k) {
        if (bsgs_run_full(left, run)) bfv_mac_fold(acc, m);
        bfv_mac_add(acc, x[k * sx], a[k * sa]);
        --left;
    }
    return bfv_mac_reduce(acc, m);
}

// he355_ckks_scalar_residues: a = the integer nearest v, ties to even; false: v is not finite or |v| >= 2^126.  mag = |a|, neg = a < 0.
inline bool poly_scalar_integer(double v, u128 &mag, bool &neg)
{
    if (!std::isfinite(v)) return false;
    double w = std::fabs(v);
    if (w >= 0x1p126) return false;
    neg = v < 0;
    if (w < 0x1p52) { // (from 2^52 on every double is an integer)
        const double f = std::floor(w), d = w - f; // exact below 2^52
        w = d > 0.5 || (d == 0.5 && std::fmod(f, 2.0) != 0.0) ? f + 1.0 : f;
    }
    if (w == 0.0) { mag = 0; neg = false; return true; }
    int e;
    const double fr = std::frexp(w, &e);                 // w = fr 2^e, fr in [0.5, 1)
    const u64 mant = (u64)std::ldexp(fr, 53);            // an integer below 2^53, exact
    const int sh = e - 53;                               // w = mant 2^sh, sh <= 73
    mag = sh >= 0 ? (u128)mant << sh : (u128)(mant >> -sh); // (w is an integer: the bits shifted out are zero)
    return true;
}
inline u64 poly_scalar_residue(u128 mag, bool neg, u64 q)
{
    const u64 r = (u64)(mag % q);
    return neg && r ? q - r : r;
}

} // namespace he355
