// cheb_core.h -- the per-lane arithmetic of the fused combine-and-rescale step (he355_combine_scalars_rescale; k_scalar_combine_row and
// k_floor_rows_combine in he355_kernels_cheb.hip), host-compilable: tests/csim/sim_cheb.cpp runs the same text on the CPU and
// tests/test_ckks_eval_mod_core_cpu.py holds it to Python integers in both forms of the u64 engine and in the fp64 engine.
//
//   A lane owns E elements of one row.  tv[r] = (sum_t a_t x_t[r] + c) mod q_i is formed as an INTEGER sum under every prime, whichever
//   engine owns it: E 128-bit sums under the run rule of poly_core.h (the constant opens the first run, bsgs_run_full cuts the later ones,
//   bfv_mac_* add and reduce).  The floor step then takes the canonical tv[r] exactly as k_floor_rows takes a word of its source slab:
//   out = (tv - x) * s^-1 mod q_i with x the transformed correction in the engine's own lazy form (ArU64 / ArF64 ::floor_fin, no addend).
//   Everything is canonical in and out, so the result is he355_rescale's of he355_combine_scalars' wherever the runs are cut.
#pragma once
#include "poly_core.h"

namespace he355 {

// the sums of a lane open on the constant's residue (0: none), which counts as the first run's first term: `left` starts at run - 1
template <int E> HE_HD void cheb_sum_open(u128 (&s)[E], u64 cst, u64 &left, u64 run)
{
    for (int r = 0; r < E; ++r) s[r] = cst;
    left = run - 1;
}
// one term: its E elements times the term's scalar under this prime
template <int E> HE_HD void cheb_sum_term(u128 (&s)[E], const u64 (&x)[E], u64 a, u64 &left, u64 run, const ModU64 &m)
{
    if (bsgs_run_full(left, run))
        for (int r = 0; r < E; ++r) bfv_mac_fold(s[r], m);
    for (int r = 0; r < E; ++r) bfv_mac_add(s[r], x[r], a);
    --left;
}
// the canonical residues of the finished sums
template <int E> HE_HD void cheb_sum_close(const u128 (&s)[E], const ModU64 &m, u64 (&tv)[E])
{
    for (int r = 0; r < E; ++r) tv[r] = bfv_mac_reduce(s[r], m);
}
// the floor step on a finished sum: (tv - x) * s^-1 mod q_i, x the forward-transformed correction (u64 engine: lazy below 4q; fp64
// engine: a centred double), fc the constants of (source prime, this prime)
template <class Ar, class FC> HE_HD u64 cheb_floor(const Ar &ar, u64 tv, typename Ar::T x, const FC &fc)
{
    return ar.floor_fin(tv, x, fc.inv, fc.inv_shoup, fc.inv_d, fc.inv_i, 0);
}

} // namespace he355
