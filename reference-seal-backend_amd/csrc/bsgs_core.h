// bsgs_core.h -- the per-element arithmetic of the baby-step/giant-step linear transform (he355_linear_transform_bsgs; k_hoist_rot_qp,
// k_bsgs_ident and k_bsgs_inner in he355_kernels_hoist.hip), host-compilable: tests/csim/sim_bsgs.cpp runs the same text on the CPU and
// tests/test_linear_transform_bsgs_core_cpu.py holds it to Python integers.
//
// A baby term T_i lives in the extended basis Q P: sigma_g of the key product of c1, with P * sigma_g(c0) folded into polynomial 0 under the
// data primes (mod_down(A + P B) = B + mod_down(A): the P-residue of P B is zero, so the rounding is A's alone).  The inner sum of a giant row
// is sum_i T_i (.) plain_i per element, formed in ONE 128-bit accumulator under the run rule of bfv_mac_core.h.  Everything is canonical in
// and out, so the result does not depend on the order of the terms or on where the runs are cut.
#pragma once
#include "bfv_mac_core.h"

namespace he355 {

// P mod q for the folded term (P < 2^63: one Barrett step)
HE_HD u64 bsgs_p_mod(u64 P, const ModU64 &m) { return barrett64(P, m); }
// one element of polynomial 0 under a data prime before the permutation: the key product's s plus P * c0 (pmq = bsgs_p_mod)
HE_HD u64 bsgs_fold_c0(u64 s, u64 c0, u64 pmq, const ModU64 &m) { return addmod(s, mulmod(c0, pmq, m), m.q); }
// the identity baby: P * c, no key product
HE_HD u64 bsgs_ident_term(u64 c, u64 pmq, const ModU64 &m) { return mulmod(c, pmq, m); }
// the giant step's accumulate: acc + v
HE_HD u64 bsgs_acc(u64 acc, u64 v, u64 q) { return addmod(acc, v, q); }

// The run rule as the kernel walks it: `left` = the terms the current 128-bit sum still takes (starts at `run`).  True: the sum is full and
// must be folded (bfv_mac_fold) before the next term; the folded residue counts as the next run's first term.
HE_HD bool bsgs_run_full(u64 &left, u64 run)
{
    if (left) return false;
    left = run - 1;
    return true;
}
// one run length for all tiles of a launch: the shortest (a shorter run is still exact; only the 60-bit primes ever reach theirs)
inline u64 bsgs_run(const u64 *q, int n_primes)
{
    u64 r = kBfvMacMaxRun;
    for (int i = 0; i < n_primes; ++i) r = bfv_mac_run(q[i]) < r ? bfv_mac_run(q[i]) : r;
    return r;
}
// One element of the inner sum: term k reads t[k * st] and p[k * sp] (the kernel walks the row's used-term list instead of strides; the
// arithmetic and the run rule are these)
HE_HD u64 bsgs_inner_sum(const u64 *t, u64 st, const u64 *p, u64 sp, u64 terms, u64 run, const ModU64 &m)
{
    u128 acc = 0;
    u64 left = run;
    for (u64 k = 0; k < terms; ++k) {
        if (bsgs_run_full(left, run)) bfv_mac_fold(acc, m);
        bfv_mac_add(acc, t[k * st], p[k * sp]);
        --left;
    }
    return bfv_mac_reduce(acc, m);
}

} // namespace he355
