// hoist_core.h -- the per-element arithmetic of the hoisted rotations' finishing kernels (he355_kernels_hoist.hip), host-compilable:
// tests/csim/sim_hoist.cpp runs the same text on the CPU and tests/test_rotate_hoisted_core_cpu.py holds it to Python integers.
//
// A hoisted rotation key-switches c1 ONCE per Galois element under the key permuted by g^-1 and applies sigma_g afterwards, to both
// polynomials: out = sigma_g(c0 + u0, u1).  Everything here works on canonical residues (below q) and returns canonical residues, so a
// sum of such terms is the same whichever order the terms were added in.
#pragma once
#include "modarith.h"

namespace he355 {

// one element of (c0 + u0, u1) before the permutation: polynomial 0 takes the input's c0 in, polynomial 1 is the key switch's alone
HE_HD u64 hoist_join(u64 u, u64 c0, bool poly0, u64 q) { return poly0 ? addmod(u, c0, q) : u; }
// NTT form: element e of the output row is element (perm[e] & 1023) of the ONE source row perm[e] >> 10 (Params::galois_perm_ntt)
HE_HD u32 hoist_src_row(u32 perm_entry) { return perm_entry >> 10; }
HE_HD u32 hoist_src_elem(u32 perm_entry) { return perm_entry & 1023u; }
// the plain sum's term: acc + plain * v (first: the sum starts here, `acc` is not read by the caller and passed as 0)
HE_HD u64 hoist_plain_term(u64 acc, u64 v, u64 plain, const ModU64 &m) { return addmod(acc, mulmod(v, plain, m), m.q); }
// coefficient form: entry g of Params::galois_gather_coeff names the source coefficient (low 31 bits) and its sign (bit 31: negated)
HE_HD u32 hoist_gather_src(u32 g) { return g & 0x7fffffffu; }
HE_HD u64 hoist_gather_sign(u64 v, u32 g, u64 q) { return (g >> 31) && v ? q - v : v; }

} // namespace he355
