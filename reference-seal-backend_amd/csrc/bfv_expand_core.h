// bfv_expand_core.h -- the per-coefficient arithmetic of the BFV monomial multiply (he355_bfv_multiply_monomial) and of the odd children
// of the oblivious query expansion (he355_bfv_expand; k_bfv_shift in he355_kernels_bfv_expand.hip): where coefficient j of in * X^e comes
// from and with which sign, and (2c - even) mod q.  Host-compilable on purpose, like bfv_mac_core.h: the HIP kernel and the test-only
// simulator (tests/csim/sim_bfv_expand.cpp, which holds these very functions to Python integers on the CPU) compile the same text.
//
//   shift  : in Z_q[X]/(X^N + 1), X^N = -1 and X^(2N) = 1, so for e in [0, 2N) coefficient j of in * X^e is coefficient k mod N of `in`,
//            k = (j - e) mod 2N, negated when k >= N.  Residues are canonical: the negative of 0 is 0.
//   odd    : a level of the expansion makes c + g and X^(-s) (c - g) of a node c, g its Galois image.  The key switch already leaves
//            even = c + g; c - g = 2c - even (mod q), so the odd child needs c and the even child only.  c, even canonical; any q < 2^63
//            (the chain's primes are below 2^61).
#pragma once
#include "device_types.h"

namespace he355 {

struct BfvShiftSrc {
    u32 idx; // coefficient of the operand, < N
    u32 neg; // 1: negated
};
// source of coefficient j < N of in * X^e, e in [0, 2N), N = 2^logN <= 2^30
HE_HD BfvShiftSrc bfv_shift_src(u32 j, u32 e, int logN)
{
    const u32 two_n = (u32)2 << logN;
    const u32 k = (j + two_n - e) & (two_n - 1);
    return BfvShiftSrc{k & ((two_n >> 1) - 1), k >> logN};
}
HE_HD u64 bfv_shift_sign(u64 x, u32 neg, u64 q) { return neg && x ? q - x : x; }
// (2c - even) mod q
HE_HD u64 bfv_expand_odd(u64 c, u64 even, u64 q) { return submod(addmod(c, c, q), even, q); }

} // namespace he355
