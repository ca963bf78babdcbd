// raise_core.h -- the per-coefficient arithmetic of the CKKS modulus raise (he355_ckks_mod_raise, he355_ckks_lift_centred; k_raise_lift and
// k_raise_cols in he355_kernels_raise.hip), host-compilable: tests/csim/sim_raise.cpp runs the same text on the CPU and
// tests/test_ckks_mod_raise_core_cpu.py holds it to Python integers.
//
//   A coefficient x, canonical under q_0, stands for the centred integer c = x (x <= (q_0 - 1) / 2) or x - q_0: bfv_lift_centred's rule
//   with t = q_0, the range of he355_plain_extend_special.  Under target prime q_j it becomes c mod q_j, in the target's own engine:
//     u64 target            bfv_lift_centred's barrett form, canonical;
//     fp64 target, q_0 < 2^52   c enters as the double it is (|c| <= (q_0 - 1) / 2, exact), re-centred only where q_0 > 2 q_j;
//     fp64 target, wider q_0    |c| = hi 2^32 + lo goes as hi * (2^32 mod q_j) + lo, one exact fp64 product (k_floor_colsn's lift_wide),
//                               re-centred (2^32 may be far above a small q_j), and takes c's sign.
//   The fp64 forms are lazy values of the fp64 engine (|v| <= q_j, the column pass's input range); their canonical residue is c mod q_j.
#pragma once
#include "bfv_level_core.h"

namespace he355 {

// c mod q_j, canonical (any q_0, q_j below 2^63)
HE_HD u64 raise_lift_u64(u64 x, u64 q0, const ModU64 &mj) { return bfv_lift_centred(x, q0, mj); }

// q_0 < 2^52: the centred c as a double, exact
HE_HD double raise_centre_f64(u64 x, u64 q0)
{
    const double v = u52_to_f64(x);
    return x > (q0 >> 1) ? v - u52_to_f64(q0) : v;
}
// ... under an fp64-engine target: as it is where |c| <= q_0 / 2 <= q_j, else re-centred
HE_HD bool raise_recentre(u64 q0, u64 qj) { return q0 > 2 * qj; }
HE_HD double raise_lift_f64(const ArF64 &ar, double c, bool recentre) { return recentre ? ar.renorm(c) : c; }
// q_0 >= 2^52 under an fp64-engine target; pow32 = 2^32 mod q_j
HE_HD double raise_lift_f64_wide(const ArF64 &ar, u64 x, u64 q0, double pow32)
{
    const bool neg = x > (q0 >> 1);
    const u64 v = neg ? q0 - x : x; // |c| < 2^63
    const double r = ar.renorm(ar.mulmod_vv((double)(u32)(v >> 32), pow32) + (double)(u32)v);
    return neg ? -r : r;
}

// The targets 1 .. L_to - 1 of one column dealt to tsplit blocks (blockIdx.y = g): block g takes g + 1, g + 1 + tsplit, ...
HE_HD int raise_first_target(int g) { return g + 1; }
// Host rule of the split: with fewer than `cus` blocks (n size 4 of them, one per quarter polynomial), min(L_to - 1, ceil(cus / blocks))
inline int raise_tsplit(u64 polys, int L_to, u64 cus)
{
    const u64 blocks = polys * 4;
    if (L_to < 3 || !blocks || blocks >= cus) return 1;
    const u64 want = (cus + blocks - 1) / blocks;
    return (int)(want < (u64)(L_to - 1) ? want : (u64)(L_to - 1));
}

} // namespace he355
