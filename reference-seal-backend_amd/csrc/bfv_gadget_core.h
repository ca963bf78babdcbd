// bfv_gadget_core.h -- the per-coefficient arithmetic of the BFV external product RGSW(m) [.] BFV(mu) -> BFV(m mu) (he355_bfv_gadget_count,
// he355_bfv_gadget_decompose, he355_bfv_gadget_decompose_ntt, he355_bfv_rgsw_encrypt, he355_bfv_external_product; kernels in
// he355_kernels_bfv_gadget.hip) and the gadget table it runs on.  Host-compilable on purpose, like bfv_digits_core.h: the HIP kernels and the
// test-only simulator (tests/csim/sim_bfv_gadget.cpp, which holds these very functions to Python integers on the CPU) compile the same text.
//
//   table   : the caller's digit width v in 1..63, b_i = bitlen(q_i), E_i = ceil(b_i / v), off_i = sum_{i' < i} E_i', E(L) = off_L: a
//             BfvDigitTab with w = v.  Gadget element G_(i,g) is 2^(g v) mod q_i under prime i and 0 under every other prime.
//   digit   : digit g of a canonical residue x is bfv_digit(x, g, v), a NON-NEGATIVE integer below 2^v (every shift is below 64:
//             g v < b_i <= 63), so x = sum_g digit_g 2^(g v) exactly and x == sum_(i,g) digit_(i,g) G_(i,g) mod q_L.  Under an output prime j
//             the same integer is used: as it is when below q_j, else (v >= b_j) after one reduction.  No centred lift: d - t is equal to d
//             mod t only, and the gadget identity holds mod q.
//   plant   : row f = k E(L) + off_i + g of RGSW(m) is an encryption of zero plus lift(m) 2^(g v) mod q_i in polynomial k under prime i;
//             lift is bfv_level_core.h's centred lift, and 2^(g v) <= 2^(b_i - 1) < q_i is canonical as it stands.
//   order   : polynomial k, prime i, digit g of ciphertext c is digit polynomial c size E(L) + k E(L) + off_i + g (bfv_digit_src's order).
//   selector: the RGSW selectors a client packs into ONE query ciphertext (he355_bfv_selector_encrypt, he355_bfv_rgsw_from_bfv).  Row
//             (k = 0, i, g) of RGSW(m), m a scalar, is planted at coefficient first_slot + b E(L) + off_i + g of polynomial 0 under prime i as
//             lift(m) 2^(g v) (2^d)^(-1) mod q_i: the expansion into 2^d children multiplies by 2^d.  The server's slot ciphertext with running
//             index c = (r n_sel + b) E + f becomes row (c / E) 2E + f of the RGSW slab [.][2E][2][L][N] (k = 0) and its product with RGSW(s)
//             row (c / E) 2E + E + f (k = 1).
#pragma once
#include "bfv_digits_core.h"
#include "bfv_level_core.h"

namespace he355 {

HE_HD bool bfv_gadget_width_ok(int v) { return v >= 1 && v <= 63; }

// host side: the table of the first L primes for digit width v (L <= kMaxPrimes, q_i < 2^63, 1 <= v <= 63)
inline BfvDigitTab bfv_gadget_table(const u64 *q, int L, int v)
{
    BfvDigitTab tab;
    tab.w = v;
    tab.L = L;
    unsigned off = 0;
    for (int i = 0; i < kMaxPrimes; ++i) {
        tab.D[i] = tab.bits[i] = 0;
        tab.off[i] = (unsigned short)off;
        if (i >= L) continue;
        const int b = bfv_bitlen(q[i]);
        tab.bits[i] = (unsigned char)b;
        tab.D[i] = (unsigned char)((b + v - 1) / v);
        off += tab.D[i];
    }
    tab.off[kMaxPrimes] = (unsigned short)off;
    tab.total = off;
    return tab;
}

// the digit (an integer below 2^v) as a canonical residue of output prime j
HE_HD u64 bfv_gadget_digit_mod(u64 d, const ModU64 &mj) { return d >= mj.q ? barrett64(d, mj) : d; }
// digit g of x under output prime j
HE_HD u64 bfv_gadget_digit(u64 x, int g, int v, const ModU64 &mj) { return bfv_gadget_digit_mod(bfv_digit(x, g, v), mj); }
// 2^(g v) under the digit's own prime: below q_i because g v <= b_i - 1
HE_HD u64 bfv_gadget_power(int g, int v) { return (u64)1 << (g * v); }
// what row (k, i, g) of RGSW(m) adds to polynomial k under prime i at a coefficient m (mod t)
HE_HD u64 bfv_gadget_plant(u64 m, u64 t, int g, int v, const ModU64 &mi)
{
    return barrett128((u128)bfv_lift_centred(m, t, mi) * bfv_gadget_power(g, v), mi);
}

// digit polynomial pf = c size E(L) + f of a batch -> the residue polynomial (c size + k) L + i it is cut from, i and g
HE_HD BfvDigitSrc bfv_gadget_src(const BfvDigitTab &tab, int size, u64 pf) { return bfv_digit_src(tab, size, pf); }
// the other way, what a block of the column pass owns: residue polynomial p = (c size + k) L + i -> its first digit polynomial
// c size E(L) + k E(L) + off_i (E_i = tab.D[i] of them follow one another)
HE_HD u64 bfv_gadget_first(const BfvDigitTab &tab, int size, u64 p)
{
    const u64 ck = p / (u64)tab.L;
    const int i = (int)(p % (u64)tab.L);
    return ck * tab.total + tab.off[i];
}

// ---- selectors packed into a query ciphertext ---------------------------------------------------------------------------------------
// host side: (2^d)^(-1) mod q, q odd: ((q + 1) / 2)^d
inline u64 bfv_selector_inv_pow2(u64 q, int d) { return bfv_level_powmod((q + 1) >> 1, (u64)d, q); }
// what selector m (mod t) adds at the coefficient of digit g under the digit's own prime: lift(m) 2^(g v) (2^d)^(-1) mod q_i
HE_HD u64 bfv_selector_value(u64 m, u64 t, int g, int v, u64 inv_pow2, const ModU64 &mi) { return mulmod(bfv_gadget_plant(m, t, g, v, mi), inv_pow2, mi); }
// slot ciphertext c = (selector) E + f -> its row of the RGSW slab [.][2E][2][L][N]: k = 0 the slot's own transform, k = 1 its product with RGSW(s)
HE_HD u64 bfv_selector_row(u64 c, u32 E, int k) { return (c / E) * 2 * E + (u64)k * E + c % E; }

// ---- the selection tree (he355_bfv_select) --------------------------------------------------------------------------------------------
// a level folds node 2p and node 2p + 1 into even + RGSW(bit) [.] (odd - even): the word whose digits the cut takes, and the tail's add.  Both are
// he355_sub / he355_add on canonical residues, so the fused level equals the composition of the public calls bit for bit.
HE_HD u64 bfv_select_diff(u64 odd, u64 even, u64 qi) { return submod(odd, even, qi); }
HE_HD u64 bfv_select_diff_digit(u64 odd, u64 even, u64 qi, int g, int v, const ModU64 &mj) { return bfv_gadget_digit(bfv_select_diff(odd, even, qi), g, v, mj); }
HE_HD u64 bfv_select_add(u64 product, u64 even, u64 qi) { return addmod(product, even, qi); }

// passes of an external product: results per pass so that a pass holds at most about `cap` digit polynomials (terms per result =
// inner 2 E(L)), never fewer than one result
HE_HD u64 bfv_gadget_pass(u64 terms, u64 n, u64 cap)
{
    u64 p = terms ? cap / terms : n;
    if (p < 1) p = 1;
    return p < n ? p : n;
}

} // namespace he355
