// bfv_merge_core.h -- the per-coefficient arithmetic of a level of the BFV ciphertext merge (he355_bfv_merge; k_bfv_merge in
// he355_kernels_bfv_expand.hip): from coefficient j of the even operand and the coefficient of the odd operand that X^s brings to j
// (bfv_shift_src of bfv_expand_core.h, e = s), the two values S = even + X^s odd and D = even - X^s odd (mod q).  Host-compilable on
// purpose, like bfv_expand_core.h: the HIP kernel and the test-only simulator (tests/csim/sim_bfv_merge.cpp, which holds this very
// function to Python integers on the CPU) compile the same text.
//
//   The definition is he355_add / he355_sub of `even` and he355_bfv_multiply_monomial(odd, s): m = bfv_shift_sign(odd, neg, q), S =
//   addmod(even, m, q), D = submod(even, m, q).  With canonical residues m is -odd exactly when neg (the negative of 0 is 0), and
//   even + (-odd) = even - odd, even - (-odd) = even + odd as canonical residues: the sign swaps the two results instead of negating
//   the operand, bit for bit the same values.  even, odd canonical; any q < 2^63.
#pragma once
#include "bfv_expand_core.h"

namespace he355 {

struct BfvMergePair {
    u64 s, d; // even + X^s odd, even - X^s odd
};
// odd: the coefficient of the odd operand that lands here; neg: 1 when the shift wrapped it past X^N = -1
HE_HD BfvMergePair bfv_merge_pair(u64 even, u64 odd, u32 neg, u64 q)
{
    const u64 a = addmod(even, odd, q), b = submod(even, odd, q);
    return neg ? BfvMergePair{b, a} : BfvMergePair{a, b};
}

} // namespace he355
