// he355_kernels_bfv_expand.hip -- multiplication by a monomial on coefficient-form BFV polynomials: he355_bfv_multiply_monomial, the odd
// children of the oblivious query expansion (he355_bfv_expand), and the sums and differences of its transpose, the ciphertext merge
// (he355_bfv_merge).  The per-coefficient arithmetic is bfv_expand_core.h and bfv_merge_core.h (host-compilable: tests/csim/sim_bfv_expand.cpp
// and sim_bfv_merge.cpp run the same text on the CPU).
//
//   k_bfv_shift<ODD, EXPAND>   streaming; a lane owns two neighbouring coefficients (2 e2, 2 e2 + 1) of one residue polynomial of the
//                        result and writes them with one 16-byte store: out = x X^e, x = in (monomial multiply) or, EXPAND, 2 in - even (the
//                        odd child X^(-s) (c - g) from the node c and its even child c + g, which the key switch has just written).
//                        An even shift keeps the pairs together: the two sources are one aligned 16-byte word of each operand, and they
//                        share a sign.  ODD (the expansion's level 0, s = 1, and odd exponents of the monomial multiply): the sources
//                        straddle two aligned words -- the lane reads both (the upper half of the one, the lower half of the other; the
//                        second is the word its neighbour's first load asks for, so every 16-byte word still leaves HBM once) and each
//                        half takes its own sign: the pair that wraps X^N = -1 has one of each.
//   k_bfv_merge<ODD>     streaming, the same lane: one level of the merge over all pairs of all results.  Pair p = k n + r (slot k < s of
//                        result r) reads its even operand at ciphertext k stride_k + r stride_r and its odd operand s stride_k behind it,
//                        and writes S = even + X^s odd and D = even - X^s odd at ciphertext p of two slabs: one aligned 16-byte load of the
//                        even operand, the shifted load(s) of the odd one exactly as k_bfv_shift's (ODD: s = 1), two 16-byte stores.  The
//                        pairs from `full` on have no partner (slots past `count`, the first level only): S = D = even.  A block lies
//                        inside one residue polynomial, so pair, slot and prime are uniform and worked out on the scalar unit.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "he355_kernels.h"
#include "bfv_expand_core.h"
#include "bfv_merge_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_expand.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

constexpr int kBlock = 256;

// residue polynomial p of every slab is [N] words at p << logN, under prime p % L
struct BfvShiftArgs {
    const u64 *in, *even; // even: EXPAND only
    u64 *out;
    u64 n_polys;
    u32 e; // exponent, < 2N
    int L, logN;
};

template <bool EXPAND> __device__ __forceinline__ ulonglong2 shift_operand(const BfvShiftArgs &A, u64 word, u64 q)
{
    ulonglong2 v = reinterpret_cast<const ulonglong2 *>(A.in)[word];
    if (EXPAND) {
        const ulonglong2 ev = reinterpret_cast<const ulonglong2 *>(A.even)[word];
        v.x = bfv_expand_odd(v.x, ev.x, q);
        v.y = bfv_expand_odd(v.y, ev.y, q);
    }
    return v;
}

template <bool ODD, bool EXPAND> __global__ void __launch_bounds__(kBlock) k_bfv_shift(BfvShiftArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 poly = gid >> (A.logN - 1);
    if (poly >= A.n_polys) return;
    const u32 e2 = (u32)(gid & (((u64)1 << (A.logN - 1)) - 1));
    const u64 q = primes[poly % A.L].q;
    const u64 base = poly << (A.logN - 1); // in 16-byte words
    const BfvShiftSrc s0 = bfv_shift_src(2 * e2, A.e, A.logN);
    ulonglong2 z;
    if (ODD) { // s0.idx is odd: the upper half of its word; the next coefficient is the lower half of another
        const BfvShiftSrc s1 = bfv_shift_src(2 * e2 + 1, A.e, A.logN);
        const ulonglong2 a = shift_operand<EXPAND>(A, base + (s0.idx >> 1), q), b = shift_operand<EXPAND>(A, base + (s1.idx >> 1), q);
        z.x = bfv_shift_sign(a.y, s0.neg, q);
        z.y = bfv_shift_sign(b.x, s1.neg, q);
    } else { // s0.idx is even, the next coefficient is its neighbour: same word, same sign
        const ulonglong2 a = shift_operand<EXPAND>(A, base + (s0.idx >> 1), q);
        z.x = bfv_shift_sign(a.x, s0.neg, q);
        z.y = bfv_shift_sign(a.y, s0.neg, q);
    }
    reinterpret_cast<ulonglong2 *>(A.out)[base + e2] = z;
}

// ciphertext c of a slab is [2][L][N] words; strides in ciphertexts
struct BfvMergeArgs {
    const u64 *in;
    u64 *S, *D;
    u64 stride_k, stride_r;
    u32 n, full; // results; the pairs below `full` have a partner
    u32 s;       // the level's shift, 2^j
    int L, logN;
};

template <bool ODD> __global__ void __launch_bounds__(kBlock) k_bfv_merge(BfvMergeArgs A, const PrimeDev *primes)
{
    const int bl = A.logN - 9; // a residue polynomial is 2^bl blocks of kBlock lanes, two coefficients each
    const u32 poly = blockIdx.x >> bl;
    const u32 e2 = ((blockIdx.x & (((u32)1 << bl) - 1)) << 8) + threadIdx.x;
    const u32 L2 = 2 * (u32)A.L;
    const u32 p = poly / L2, c = poly - p * L2;
    const u32 k = p / A.n, r = p - k * A.n;
    const u64 q = primes[c % (u32)A.L].q;
    const ulonglong2 *in = reinterpret_cast<const ulonglong2 *>(A.in);
    const u64 ev = ((k * A.stride_k + r * A.stride_r) * L2 + c) << (A.logN - 1); // in 16-byte words
    const ulonglong2 x = in[ev + e2];
    ulonglong2 zs = x, zd = x;
    if (p < A.full) {
        const u64 od = ev + ((A.s * A.stride_k * L2) << (A.logN - 1));
        const BfvShiftSrc s0 = bfv_shift_src(2 * e2, A.s, A.logN);
        BfvMergePair lo, hi;
        if (ODD) { // as k_bfv_shift: the upper half of one word, the lower half of another, a sign each
            const BfvShiftSrc s1 = bfv_shift_src(2 * e2 + 1, A.s, A.logN);
            const ulonglong2 a = in[od + (s0.idx >> 1)], b = in[od + (s1.idx >> 1)];
            lo = bfv_merge_pair(x.x, a.y, s0.neg, q);
            hi = bfv_merge_pair(x.y, b.x, s1.neg, q);
        } else {
            const ulonglong2 a = in[od + (s0.idx >> 1)];
            lo = bfv_merge_pair(x.x, a.x, s0.neg, q);
            hi = bfv_merge_pair(x.y, a.y, s0.neg, q);
        }
        zs.x = lo.s; zs.y = hi.s;
        zd.x = lo.d; zd.y = hi.d;
    }
    const u64 o = ((u64)poly << (A.logN - 1)) + e2;
    reinterpret_cast<ulonglong2 *>(A.S)[o] = zs;
    reinterpret_cast<ulonglong2 *>(A.D)[o] = zd;
}

} // namespace

void launch_bfv_merge(const KernelEnv &env, int L, u64 n, u64 s, u64 full, const u64 *in, u64 stride_k, u64 stride_r, u64 *S, u64 *D)
{
    const u64 pairs = s * n;
    if (!pairs) return;
    const int logN = env.logn1 + kRowLog;
    if (L < 1 || L > kMaxPrimes || logN < 9 || s < 1 || s > ((u64)1 << (logN - 1)) || (s & (s - 1)) || full > pairs) throw std::invalid_argument("merge: level or shift out of range");
    if (n > 0x7fffffffull || pairs > (0x7fffffffull >> (logN - 9)) / (2 * (u64)L)) throw std::invalid_argument("merge: too many polynomials for one launch");
    BfvMergeArgs A{};
    A.in = in; A.S = S; A.D = D; A.stride_k = stride_k; A.stride_r = stride_r; A.n = (u32)n; A.full = (u32)full; A.s = (u32)s; A.L = L; A.logN = logN;
    const dim3 g((unsigned)((pairs * 2 * L) << (logN - 9))), b(kBlock);
    if (s == 1) hipLaunchKernelGGL((k_bfv_merge<true>), g, b, 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL((k_bfv_merge<false>), g, b, 0, env.stream, A, env.primes);
}

void launch_bfv_shift(const KernelEnv &env, int L, u64 n_polys, const u64 *in, const u64 *even, u32 e, u64 *out)
{
    if (!n_polys) return;
    const int logN = env.logn1 + kRowLog;
    if (L < 1 || L > kMaxPrimes || e >= ((u32)2 << logN)) throw std::invalid_argument("monomial multiply: level or exponent out of range");
    const u64 blocks = (n_polys << (logN - 1)) / kBlock; // N / 2 is a multiple of kBlock: a block lies inside one polynomial
    if (blocks > 0x7fffffffull) throw std::invalid_argument("monomial multiply: too many polynomials for one launch");
    BfvShiftArgs A{};
    A.in = in; A.even = even; A.out = out; A.n_polys = n_polys; A.e = e; A.L = L; A.logN = logN;
    const dim3 g((unsigned)blocks), b(kBlock);
    const bool odd = e & 1;
    if (even) {
        if (odd) hipLaunchKernelGGL((k_bfv_shift<true, true>), g, b, 0, env.stream, A, env.primes);
        else hipLaunchKernelGGL((k_bfv_shift<false, true>), g, b, 0, env.stream, A, env.primes);
    } else {
        if (odd) hipLaunchKernelGGL((k_bfv_shift<true, false>), g, b, 0, env.stream, A, env.primes);
        else hipLaunchKernelGGL((k_bfv_shift<false, false>), g, b, 0, env.stream, A, env.primes);
    }
}

} // namespace HE355_KNS
} // namespace he355
