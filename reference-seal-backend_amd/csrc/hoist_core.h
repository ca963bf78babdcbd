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

// ---- the lazy plain sum (k_hoist_acc_qp): the key products stay in the extended basis Q P, are permuted, multiplied by plaintexts that carry
// a residue under the special prime and accumulated there; ONE mod-down per sum (he355_rotate_hoisted_plain_sum_lazy) ----------------------
// tile idx of a level-L accumulator: the data primes 0 .. L - 1, then the special prime K - 1 (row L of a [L + 1][N] plaintext)
HE_HD int hoist_qp_prime(int idx, int L, int K) { return idx < L ? idx : K - 1; }
// one term of an accumulator (A in Q P, B in Q): acc + plain * v, canonical in and out, so the terms may come in any order (first: the
// accumulator starts here, `acc` is passed as 0)
HE_HD u64 hoist_acc_term(u64 acc, u64 v, u64 plain, const ModU64 &m) { return addmod(acc, mulmod(v, plain, m), m.q); }
// The special prime's key product reaches the accumulate kernel after k_k3's inverse row pass; the wave runs the forward row pass on it.
// Ten Gentleman-Sande stages without N^-1 and ten Cooley-Tukey stages make 2^10 times the row: fix = 1024^-1 mod q takes that out
// (ten halvings of 1 mod the odd q).  N = 1024: the inverse pass carried N^-1 itself and nothing is left to take out.
HE_HD u64 hoist_row_pass_fix(u64 q)
{
    u64 x = 1;
    for (int s = 0; s < 10; ++s) x = (x & 1) ? (x >> 1) + (q >> 1) + 1 : x >> 1;
    return x;
}
HE_HD u64 hoist_sp_unscale(u64 v, u64 fix, const ModU64 &m) { return mulmod(v, fix, m); }
// he355_plain_extend_special: c, a residue under q0 (half0 = floor(q0 / 2)), centred into (-q0 / 2, q0 / 2] and reduced mod m.q
HE_HD u64 hoist_centred_mod(u64 c, u64 q0, u64 half0, const ModU64 &m)
{
    if (c <= half0) return barrett64(c, m);
    const u64 r = barrett64(q0 - c, m); // -(q0 - c)
    return r ? m.q - r : 0;
}

} // namespace he355
