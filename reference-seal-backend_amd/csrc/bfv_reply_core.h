// bfv_reply_core.h -- the arithmetic of BFV reply compression: an L = 1 ciphertext switched to the moduli 2^k0 (c0) and 2^k1 (c1) and
// bit-packed, and the client's decryption of such a reply (he355_bfv_reply_bytes, he355_bfv_reply_safe_bits, he355_bfv_reply_compress,
// he355_bfv_reply_decrypt; kernels in he355_kernels_bfv_reply.hip).  Host-compilable on purpose, like bfv_bytes_core.h: the HIP kernels and
// the test-only simulator (tests/csim/sim_bfv_reply.cpp) compile the same text.  Exact integers throughout, no tolerance.
//
//   switch     : q = q_0, the modulus at L = 1 (odd: no ties).  For x in [0, q): cut_k(x) = floor((x 2^k + floor(q / 2)) / q) mod 2^k; an x
//                that rounds to 2^k wraps to 0.  The numerator has up to 118 bits; it is never formed.  With c = floor(2^(64+k) / q) (one
//                word: 2^k < q), e = floor(x c / 2^64) is floor(x 2^k / q) or one less (x c / 2^64 falls short of x 2^k / q by less than
//                q / 2^64 < 1), so r = x 2^k - e q lies in [0, 2 q) and is exact in 64 bits, and the quotient is e plus one for each of
//                r + floor(q / 2) >= q and >= 2 q: a reciprocal with correction, one high and one low product per coefficient.
//   layout     : one reply is the little-endian bit string of c0's N fields of k0 bits, then c1's N fields of k1 bits, coefficient e at
//                bit e k.  N >= 1024, so each half is whole 64-bit words, N k / 64 of them, and a reply is N (k0 + k1) / 8 bytes.  Output
//                word j of a half holds coefficients floor(64 j / k) .. floor((64 j + 63) / k), the first shifted down when it began in
//                word j - 1 (the byte codec's word rule; one owner per word, no atomics, no partial stores).  The field at bit p = e k lies
//                in words p >> 6 and, when it reaches into it, (p >> 6) + 1; the last field of a half ends with the half's last word.
//   decryption : y0, y1 unpacked.  y1 centred, y1 - 2^k1 where y1 >= 2^(k1 - 1), lifted mod q: the operand of the negacyclic product with
//                the secret key at prime 0, whose centred representative is w.  z = (y0 2^(k1 - k0) + w) mod 2^k1,
//                M = floor((t z + 2^(k1 - 1)) / 2^k1), the plaintext coefficient is M mod t (M <= t: M = t reduces to 0), the residue is
//                |t z - M 2^k1| <= 2^(k1 - 1); a reply's noise_bits is the bit length of its largest residue and its budget
//                max(0, k1 - noise_bits - 1): bfv_noise_budget_of with 2^k1 in the place of q.
//   widths     : accepted 2 <= k0 <= k1 and N 2^(k1 - 1) <= (q - 1) / 2 (then w is the integer product for every ternary key);
//                safe k0 = bitlen(t) + 2, k1 = bitlen(t) + 2 + log2 N (every coefficient of an input with at least 2 bits of invariant
//                noise budget at L = 1 decrypts correctly under a ternary key: |v'| <= 2^-3 + t 2^-(k0+1) + t N 2^-(k1+1) < 3/8).
#pragma once
#include "bfv_digits_core.h"

namespace he355 {

// the switch to 2^k under q: q, floor(q / 2), floor(2^(64+k) / q), and floor(2^32 / k) + 1 (the word rule's division by k as a product)
struct BfvReplyCut {
    u64 q, half, recip;
    u32 kinv;
    int k;
};
// host side: the constants of one accepted width (2 <= k, 2^k < q)
inline BfvReplyCut bfv_reply_cut_of(u64 q, int k)
{
    BfvReplyCut c;
    c.q = q; c.half = q >> 1; c.recip = (u64)(((u128)1 << (64 + k)) / q); c.kinv = (u32)((((u64)1 << 32) / (u64)k) + 1); c.k = k;
    return c;
}
// ---- widths and sizes -------------------------------------------------------------------------------------------------------------------
HE_HD bool bfv_reply_widths_ok(u64 N, u64 q, int k0, int k1)
{
    if (k0 < 2 || k0 > k1 || k1 > 62) return false;
    return ((q - 1) >> 1) / N >= ((u64)1 << (k1 - 1)); // N 2^(k1 - 1) <= (q - 1) / 2, N a power of two
}
HE_HD u64 bfv_reply_half_words(u64 N, int k) { return N / 64 * (u64)k; }
HE_HD u64 bfv_reply_size(u64 N, int k0, int k1) { return 8 * (bfv_reply_half_words(N, k0) + bfv_reply_half_words(N, k1)); } // bytes
HE_HD void bfv_reply_safe(u64 N, u64 t, int &k0, int &k1)
{
    k0 = bfv_bitlen(t) + 2;
    k1 = k0 + bfv_bitlen(N) - 1;
}

// ---- the switch ---------------------------------------------------------------------------------------------------------------------------
HE_HD u64 bfv_reply_cut(u64 x, const BfvReplyCut &c)
{
    u64 e = mulhi64(x, c.recip);
    const u64 r = (x << c.k) - e * c.q + c.half; // (mod 2^64; the value is below 2 q + q / 2 < 2^63)
    e += (r >= c.q) + (r >= 2 * c.q);
    return e & bfv_digit_mask(c.k);
}

// ---- fields over whole words ----------------------------------------------------------------------------------------------------------------
// floor(p / k) for a bit position p < 2^26 (N k <= 2^15 62): p kinv / 2^32 exceeds p / k by less than 2^-6 < 1 / k
HE_HD u32 bfv_reply_div(u32 p, const BfvReplyCut &c) { return (u32)(((u64)p * c.kinv) >> 32); }
// output word j < N k / 64 of the half whose N coefficients (canonical residues mod q) are coef[]
HE_HD u64 bfv_reply_pack_word(const u64 *coef, u32 j, const BfvReplyCut &c)
{
    const u32 lo = 64 * j, e0 = bfv_reply_div(lo, c), e1 = bfv_reply_div(lo + 63, c); // (e1 <= N - 1: the half ends with its last word)
    u64 out = 0;
    for (u32 e = e0; e <= e1; ++e) {
        const u64 v = bfv_reply_cut(coef[e], c);
        const u32 p = e * (u32)c.k;
        out |= p < lo ? v >> (lo - p) : v << (p - lo); // (lo - p < k <= 62, p - lo <= 63)
    }
    return out;
}
// field e < N of the half whose words are w[]
HE_HD u64 bfv_reply_field(const u64 *w, u32 e, int k)
{
    const u32 p = e * (u32)k, j = p >> 6;
    const int r = (int)(p & 63);
    u64 v = w[j] >> r;
    if (r + k > 64) v |= w[j + 1] << (64 - r); // (r >= 3 here: the shift is below 64; the half's last field ends on bit 63)
    return v & bfv_digit_mask(k);
}

// ---- centring and the lift mod q ------------------------------------------------------------------------------------------------------------
// y1 < 2^k1 centred, as a canonical residue mod q (2^(k1 - 1) < q / 2)
HE_HD u64 bfv_reply_lift(u64 y1, int k1, u64 q) { return y1 >> (k1 - 1) ? q - (((u64)1 << k1) - y1) : y1; }

// ---- the final rounding with its residue --------------------------------------------------------------------------------------------------
struct BfvReplyCoef {
    u64 m;    // the plaintext coefficient, M mod t
    int bits; // the bit length of |t z - M 2^k1|
};
// w: the product's residue mod q, centred here
HE_HD BfvReplyCoef bfv_reply_round(u64 y0, u64 w, int k0, int k1, u64 q, u64 t)
{
    const u64 wc = w > (q >> 1) ? w - q : w; // two's complement: the sum below is taken mod 2^k1 <= 2^62
    const u64 z = ((y0 << (k1 - k0)) + wc) & bfv_digit_mask(k1);
    const u64 half = (u64)1 << (k1 - 1);
    const u128 tz = (u128)t * z + half;
    const u64 M = (u64)(tz >> k1), low = (u64)tz & bfv_digit_mask(k1);
    BfvReplyCoef c;
    c.m = M >= t ? M - t : M;
    c.bits = bfv_bitlen(low >= half ? low - half : half - low);
    return c;
}

} // namespace he355
