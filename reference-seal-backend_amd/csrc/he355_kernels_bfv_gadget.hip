// he355_kernels_bfv_gadget.hip -- the BFV external product RGSW(m) [.] BFV(mu) -> BFV(m mu): he355_bfv_gadget_decompose_ntt,
// he355_bfv_rgsw_encrypt, he355_bfv_external_product; the selection tree he355_bfv_select; and the selectors a client packs into one query ciphertext:
// he355_bfv_selector_encrypt, he355_bfv_rgsw_encrypt_secret, he355_bfv_rgsw_from_bfv.  The per-coefficient arithmetic is bfv_gadget_core.h and bfv_mac_core.h
// (host-compilable: tests/csim/sim_bfv_gadget.cpp and sim_bfv_select.cpp run the same text on the CPU).
//
//   k_bfv_gadget_cols_fwd<LOGN1>   N >= 2048: the forward COLUMN pass of every digit polynomial of one ciphertext residue.  A block owns a
//                        quarter of the 1024 columns of one residue polynomial (c, k, i); a lane owns one stride-1024 column and loads its
//                        N / 1024 ciphertext words ONCE.  For each digit g < E_i and each output prime j < L it cuts the digit (the plain
//                        integer below 2^v, reduced once where it is not below q_j), runs k_cols_fwd's lane program with the engine that
//                        owns j (fp64 or u64, the u64 one in this build's form) and stores the raw column into digit polynomial
//                        (c 2E + k E + off_i + g, j).  The row pass is the existing k_rows_fwd, in place.  Registers: the N / 1024 source
//                        words and one working column, as k_bfv_digits_cols_fwd.  The ciphertexts are read where they lie: ciphertext
//                        (a, b) at index a stride_a + b stride_b.
//   k_bfv_gadget_spread  N = 1024 (no column pass) and batches too small to fill the chip with column-pass blocks: streaming; a lane owns two
//                        coefficients of one residue polynomial, one 16-byte load, E_i L 16-byte stores of the digits under every output prime, coefficient form; the existing transform follows in place.
//   k_bfv_gadget_mac     batched over results; a lane owns two coefficients (16 bytes per access) of residue j of result r, both
//                        polynomials.  Per term (kappa, f) it loads one digit word and two RGSW row words and feeds four 128-bit sums,
//                        folded per bfv_mac_run of prime j; canonical residues out.  Block = (residue, coefficient block, result), the
//                        result fastest: with one selector row for all results (rg_stride_r == 0) the blocks that read the same row
//                        words are neighbours in the grid, as in k_bfv_plain_mac.
//   k_bfv_rgsw_plant     streaming; a lane owns two coefficients of one output residue polynomial (row, k', i'): it reads the encryption of
//                        zero (level L_in >= L, cut to the first L primes) and, where (k', i') is the row's own (k, i), adds
//                        lift(m) 2^(g v) mod q_i.  In place when L_in == L.  The existing forward transform follows.
// he355_bfv_rgsw_from_bfv runs the same kernels in their OWN form (a template flag; the plain form compiles what it compiled before):
//   k_bfv_gadget_cols_fwd<LOGN1, true>  also runs the lane program on the ciphertext words it holds, under the residue's own prime, and stores
//                        that raw column into row bfv_selector_row(c, E, 0) of the RGSW slab: the k = 0 rows cost no second read of the
//                        children.  The working column is the one the digits use, so the register count is the plain form's.
//   k_bfv_gadget_spread<true>           also stores the 16 bytes it loaded into that row, coefficient form.
//   k_bfv_gadget_mac<true>              one term list per slot ciphertext (inner = 1, all of them against RGSW(s)); the NTT-form sums go
//                        straight to row bfv_selector_row(c, E, 1).
//   k_bfv_selector_plant streaming; a lane owns two coefficients of one output residue polynomial (r, k, i) of the query ciphertexts: the
//                        encryption of zero cut to L primes and, in polynomial 0 at a coefficient that is a slot of a digit of prime i,
//                        bfv_selector_value of the slot's selector.
//   k_bfv_secret_plain   the secret key's coefficients under prime 0 (0, 1, q_0 - 1) -> 0, 1, t - 1.
// he355_bfv_select (one level = a pass loop over all pairs of all results) has kernel bodies of its own: as template forms of the kernels above
// they changed the OWN instantiations' registers (profiles/bfv_select.txt), and those must compile what they compiled before:
//   k_bfv_select_cols_fwd<LOGN1>, k_bfv_select_spread   the cut of odd - even: a lane loads the two nodes' words from their own addresses
//                        and cuts the digits of submod(odd, even, q_i); the difference is never stored.
//   k_bfv_select_mac     k_bfv_gadget_mac with inner = 1 whose "result" is a pair: pair c takes the selector row of result c / group, so the
//                        blocks that share a row stay neighbours in the grid.
//   k_bfv_select_cols_inv<LOGN1>  k_cols_inv's lane program on the sums' raw rows; after to_canon it adds the even node's word and stores the
//                        next level's node.  k_bfv_select_add: the same add for N = 1024, whose sums launch_ntt_inverse leaves as
//                        coefficients.  k_bfv_select_copy: the node without a partner, one launch per level that has one.
// Launches: kernel_common.inc's dispatch_logn1 picks the LOGN1 instantiation, streaming_grid / grid_blocks size and bound the grids.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "bfv_gadget_core.h"
#include "bfv_mac_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_gadget.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// ciphertext (a, b), a < n_a, b < n_b, at index a stride_a + b stride_b of `in`, [size][L][N] each; digit polynomials
// [(a n_b + b) size E + f][L][N] of `out`
struct BfvGadgetCutArgs {
    const u64 *in;
    u64 *out;
    u64 n_b, stride_a, stride_b;
    u64 n_polys; // n_a n_b size L residue polynomials
    int L, size, logN;
    BfvDigitTab tab;
    // the batch is ciphertexts first .. of the (a, b) order; OWN form (size 2): ciphertext c of that order is also written, transformed as
    // the digits are, to row bfv_selector_row(c, own_E, 0) of own [.][2 own_E][2][L][N]
    u64 first;
    u64 *own;
    u32 own_E;
};

// residue polynomial p of the batch -> its words
__device__ __forceinline__ const u64 *gadget_src(const BfvGadgetCutArgs &A, u64 p)
{
    const u64 polys = (u64)A.size * A.L, c = A.first + p / polys, rest = p % polys;
    const u64 at = (c / A.n_b) * A.stride_a + (c % A.n_b) * A.stride_b;
    return A.in + ((at * polys + rest) << A.logN);
}
// OWN form: where residue polynomial p of the batch goes in the RGSW slab
__device__ __forceinline__ u64 *gadget_own_dst(const BfvGadgetCutArgs &A, u64 p)
{
    const u64 polys = 2 * (u64)A.L;
    return A.own + ((bfv_selector_row(A.first + p / polys, A.own_E, 0) * polys + p % polys) << A.logN);
}

template <int LOGN1, bool OWN>
__global__ void __launch_bounds__(kBlock) k_bfv_gadget_cols_fwd(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 p = blockIdx.x >> 2; // residue polynomial (c size + k) L + i
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, A.size, p);
    const u64 *src = gadget_src(A, p);
    u64 w[N1];
#pragma unroll
    for (int a = 0; a < N1; ++a) w[a] = src[(a << kRowLog) + col];
    if (OWN) { // the ciphertext's own column under its own prime: k_cols_fwd's program on the words already here
        const PrimeDev &P = primes[i];
        u64 *dst = gadget_own_dst(A, p);
        if (P.f64) {
            const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
            double x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(w[a]);
            col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
        } else {
            const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
            u64 x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = w[a];
            col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
        }
    }
    for (int g = 0; g < E; ++g) {
        for (int j = 0; j < A.L; ++j) {
            const PrimeDev &P = primes[j];
            const ModU64 mj = make_modu(P);
            u64 *dst = A.out + (((f0 + g) * A.L + j) << (LOGN1 + kRowLog));
            if (P.f64) {
                const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
                double x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(bfv_gadget_digit(w[a], g, v, mj));
                col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
            } else {
                const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
                u64 x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = bfv_gadget_digit(w[a], g, v, mj);
                col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
            }
        }
    }
}

template <bool OWN>
__global__ void __launch_bounds__(kBlock) k_bfv_gadget_spread(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, A.size, p);
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(gadget_src(A, p))[e2];
    if (OWN) reinterpret_cast<ulonglong2 *>(gadget_own_dst(A, p))[e2] = x;
    for (int g = 0; g < E; ++g)
        for (int j = 0; j < A.L; ++j) {
            const ModU64 mj = make_modu(primes[j]);
            reinterpret_cast<ulonglong2 *>(A.out + (((f0 + g) * A.L + j) << A.logN))[e2] =
                make_ulonglong2(bfv_gadget_digit(x.x, g, v, mj), bfv_gadget_digit(x.y, g, v, mj));
        }
}

// result r < n: digits [r][inner][rows][L][N] (NTT form), RGSW (r, kappa) at index r rg_stride_r + kappa rg_stride_k, [rows][2][L][N] each
struct BfvGadgetMacArgs {
    const u64 *dig, *rgsw;
    u64 *out;
    u64 n, rg_stride_r, rg_stride_k;
    u32 inner, rows, pairs_blocks; // rows = 2 E(L); pairs_blocks = N / 2 / kBlock
    int L, logN;
    u32 run[kMaxPrimes]; // bfv_mac_run of prime j
    // OWN form: result r is slot ciphertext first + r, and goes to row bfv_selector_row(first + r, own_E, 1) of out [.][2 own_E][2][L][N]
    u64 first;
    u32 own_E;
};

template <bool OWN>
__global__ void __launch_bounds__(kBlock) k_bfv_gadget_mac(BfvGadgetMacArgs A, const PrimeDev *primes)
{
    // block = (residue j, coefficient block, result), the result fastest
    const u64 r = blockIdx.x % A.n;
    const u32 rest = (u32)(blockIdx.x / A.n), eb = rest % A.pairs_blocks;
    const int j = (int)(rest / A.pairs_blocks);
    const u64 e2 = (u64)eb * kBlock + threadIdx.x;
    const u64 N = (u64)1 << A.logN, LN = (u64)A.L << A.logN;
    const ModU64 m = bfv_modu(primes[j]);
    const u64 run = A.run[j];
    // in 16-byte words: a digit polynomial is LN / 2 after the one before it, an RGSW row LN, its second polynomial LN / 2 into the row
    const ulonglong2 *pd = reinterpret_cast<const ulonglong2 *>(A.dig + r * A.inner * A.rows * LN + (u64)j * N) + e2;
    const ulonglong2 *pr = reinterpret_cast<const ulonglong2 *>(A.rgsw + r * A.rg_stride_r * A.rows * 2 * LN + (u64)j * N) + e2;
    const u64 step_k = A.rg_stride_k * A.rows * LN, half = LN / 2;

    u128 acc[2][2] = {{0, 0}, {0, 0}}; // [polynomial][coefficient]
    u64 left = run;                    // terms the running sums still take
    for (u32 kappa = 0; kappa < A.inner; ++kappa) {
        const ulonglong2 *row = pr + kappa * step_k;
        u32 f = 0;
        while (f < A.rows) {
            if (!left) { // the sums' residues start the next run as one term
                bfv_mac_fold(acc[0][0], m); bfv_mac_fold(acc[0][1], m);
                bfv_mac_fold(acc[1][0], m); bfv_mac_fold(acc[1][1], m);
                left = run - 1;
            }
            const u32 end = A.rows - f < left ? A.rows : f + (u32)left;
            left -= end - f;
#pragma unroll 2
            for (; f < end; ++f) {
                const ulonglong2 d = pd[f * half], a = row[f * LN], b = row[f * LN + half];
                bfv_mac_add(acc[0][0], a.x, d.x);
                bfv_mac_add(acc[0][1], a.y, d.y);
                bfv_mac_add(acc[1][0], b.x, d.x);
                bfv_mac_add(acc[1][1], b.y, d.y);
            }
        }
        pd += A.rows * half;
    }
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(A.out + (OWN ? bfv_selector_row(A.first + r, A.own_E, 1) : r) * 2 * LN + (u64)j * N) + e2;
    po[0] = make_ulonglong2(bfv_mac_reduce(acc[0][0], m), bfv_mac_reduce(acc[0][1], m));
    po[half] = make_ulonglong2(bfv_mac_reduce(acc[1][0], m), bfv_mac_reduce(acc[1][1], m));
}

// he355_bfv_select: the batch is PAIRS.  Residue polynomial p of the batch belongs to pair c = first + p / (2 L) = (a, b) = (c / n_b, c % n_b), whose
// even node is the ciphertext at index a stride_a + 2 b stride_b and whose odd node lies stride_b behind it: -> the even node's words, and the
// distance in words to the odd node's
__device__ __forceinline__ const u64 *select_even(const BfvGadgetCutArgs &A, u64 p, u64 &to_odd)
{
    const u64 polys = 2 * (u64)A.L, c = A.first + p / polys, rest = p % polys;
    const u64 at = (c / A.n_b) * A.stride_a + 2 * (c % A.n_b) * A.stride_b;
    to_odd = (A.stride_b * polys) << A.logN;
    return A.in + ((at * polys + rest) << A.logN);
}
// The DIFF form of k_bfv_gadget_cols_fwd, a kernel body of its own (the shared template changed the OWN instantiations' registers:
// profiles/bfv_select.txt): a lane loads its words of the odd and of the even node from their own addresses and cuts the digits of odd - even;
// the difference is never stored.  The rest is k_bfv_gadget_cols_fwd's text.
template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_select_cols_fwd(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 p = blockIdx.x >> 2; // residue polynomial (pair 2 + k) L + i
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, 2, p), qi = primes[i].q;
    u64 to_odd;
    const u64 *even = select_even(A, p, to_odd), *odd = even + to_odd;
    u64 w[N1];
#pragma unroll
    for (int a = 0; a < N1; ++a) w[a] = bfv_select_diff(odd[(a << kRowLog) + col], even[(a << kRowLog) + col], qi);
    for (int g = 0; g < E; ++g) {
        for (int j = 0; j < A.L; ++j) {
            const PrimeDev &P = primes[j];
            const ModU64 mj = make_modu(P);
            u64 *dst = A.out + (((f0 + g) * A.L + j) << (LOGN1 + kRowLog));
            if (P.f64) {
                const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
                double x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(bfv_gadget_digit(w[a], g, v, mj));
                col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
            } else {
                const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
                u64 x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = bfv_gadget_digit(w[a], g, v, mj);
                col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
            }
        }
    }
}

// the DIFF form of k_bfv_gadget_spread: two 16-byte loads, the digits of odd - even under every output prime
__global__ void __launch_bounds__(kBlock) k_bfv_select_spread(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, 2, p), qi = primes[i].q;
    u64 to_odd;
    const u64 *even = select_even(A, p, to_odd);
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(even)[e2], y = reinterpret_cast<const ulonglong2 *>(even + to_odd)[e2];
    for (int g = 0; g < E; ++g)
        for (int j = 0; j < A.L; ++j) {
            const ModU64 mj = make_modu(primes[j]);
            reinterpret_cast<ulonglong2 *>(A.out + (((f0 + g) * A.L + j) << A.logN))[e2] =
                make_ulonglong2(bfv_select_diff_digit(y.x, x.x, qi, g, v, mj), bfv_select_diff_digit(y.y, x.y, qi, g, v, mj));
        }
}

// k_bfv_gadget_mac's plain form with inner = 1 for he355_bfv_select, a kernel body of its own: the "result" is pair `first` + r of a level,
// digits [pair][rows][L][N], and its RGSW ciphertext is the one at index ((first + r) / group) rg_stride_r, group = the pairs per result --
// the pairs of one result are neighbours in the grid, so the blocks that read the same selector row words still are.  out [pair][2][L][N].
struct BfvSelectMacArgs {
    const u64 *dig, *rgsw;
    u64 *out;
    u64 n, rg_stride_r, first, group;
    u32 rows, pairs_blocks;
    int L, logN;
    u32 run[kMaxPrimes];
};
__global__ void __launch_bounds__(kBlock) k_bfv_select_mac(BfvSelectMacArgs A, const PrimeDev *primes)
{
    const u64 r = blockIdx.x % A.n;
    const u32 rest = (u32)(blockIdx.x / A.n), eb = rest % A.pairs_blocks;
    const int j = (int)(rest / A.pairs_blocks);
    const u64 e2 = (u64)eb * kBlock + threadIdx.x;
    const u64 N = (u64)1 << A.logN, LN = (u64)A.L << A.logN, half = LN / 2;
    const ModU64 m = bfv_modu(primes[j]);
    const u64 run = A.run[j];
    const ulonglong2 *pd = reinterpret_cast<const ulonglong2 *>(A.dig + r * A.rows * LN + (u64)j * N) + e2;
    const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(A.rgsw + ((A.first + r) / A.group) * A.rg_stride_r * A.rows * 2 * LN + (u64)j * N) + e2;

    u128 acc[2][2] = {{0, 0}, {0, 0}}; // [polynomial][coefficient]
    u64 left = run;
    u32 f = 0;
    while (f < A.rows) {
        if (!left) { // the sums' residues start the next run as one term
            bfv_mac_fold(acc[0][0], m); bfv_mac_fold(acc[0][1], m);
            bfv_mac_fold(acc[1][0], m); bfv_mac_fold(acc[1][1], m);
            left = run - 1;
        }
        const u32 end = A.rows - f < left ? A.rows : f + (u32)left;
        left -= end - f;
#pragma unroll 2
        for (; f < end; ++f) {
            const ulonglong2 d = pd[f * half], a = row[f * LN], b = row[f * LN + half];
            bfv_mac_add(acc[0][0], a.x, d.x);
            bfv_mac_add(acc[0][1], a.y, d.y);
            bfv_mac_add(acc[1][0], b.x, d.x);
            bfv_mac_add(acc[1][1], b.y, d.y);
        }
    }
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(A.out + r * 2 * LN + (u64)j * N) + e2;
    po[0] = make_ulonglong2(bfv_mac_reduce(acc[0][0], m), bfv_mac_reduce(acc[0][1], m));
    po[half] = make_ulonglong2(bfv_mac_reduce(acc[1][0], m), bfv_mac_reduce(acc[1][1], m));
}

// The tail of a level of he355_bfv_select and its pass-through copy.  Pair c = first + (the pass's pair index) is (r, b) = (c / group, c % group):
// its even node is the ciphertext at index r stride_a + 2 b stride_b of `nodes`, its sums are `sums` [pair of the pass][2][L][N], and the next
// level's node (r, b) is the ciphertext at index r out_stride + b of `out`.
struct BfvSelectTailArgs {
    const u64 *sums, *nodes;
    u64 *out;
    u64 first, group, stride_a, stride_b, out_stride;
    u64 n_polys; // residue polynomials of the launch: pairs 2 L (the copy: n 2 L)
    int L, logN;
};
// residue polynomial p = (pair of the pass) 2 L + (k L + i) -> where its even node's and its output's words start
__device__ __forceinline__ void select_tail_at(const BfvSelectTailArgs &A, u64 p, const u64 *&even, u64 *&dst)
{
    const u64 polys = 2 * (u64)A.L, c = A.first + p / polys, rest = p % polys, r = c / A.group, b = c % A.group;
    even = A.nodes + (((r * A.stride_a + 2 * b * A.stride_b) * polys + rest) << A.logN);
    dst = A.out + (((r * A.out_stride + b) * polys + rest) << A.logN);
}
// k_cols_inv's lane program on the sums' raw rows; after to_canon the even node's word is added and the next level's node stored
template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_select_cols_inv(BfvSelectTailArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 p = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const PrimeDev &P = primes[(int)(p % (u64)A.L)];
    const u64 *src = A.sums + (p << (LOGN1 + kRowLog)), *even;
    u64 *dst;
    select_tail_at(A, p, even, dst);
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = bfv_select_add(ar.to_canon(x[a]), even[(a << kRowLog) + col], P.q);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = bfv_select_add(ar.to_canon(x[a]), even[(a << kRowLog) + col], P.q);
    }
}
// N = 1024 (no column pass): the sums are coefficients already (launch_ntt_inverse); streaming, a lane owns two coefficients.  k_addsub's
// indexer cannot say "node 2 b of result r", so the add is this kernel's
__global__ void __launch_bounds__(kBlock) k_bfv_select_add(BfvSelectTailArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 q = primes[(int)(p % (u64)A.L)].q;
    const u64 *even;
    u64 *dst;
    select_tail_at(A, p, even, dst);
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.sums + (p << A.logN))[e2], y = reinterpret_cast<const ulonglong2 *>(even)[e2];
    reinterpret_cast<ulonglong2 *>(dst)[e2] = make_ulonglong2(bfv_select_add(x.x, y.x, q), bfv_select_add(x.y, y.y, q));
}
// the node without a partner (node 2 group of every result, where the level has an odd number of nodes) -> node `group` of the next level;
// group == 0: a level of one node, he355_bfv_select's count == 1
__global__ void __launch_bounds__(kBlock) k_bfv_select_copy(BfvSelectTailArgs A)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 polys = 2 * (u64)A.L, r = p / polys, rest = p % polys;
    reinterpret_cast<ulonglong2 *>(A.out + (((r * A.out_stride + A.group) * polys + rest) << A.logN))[e2] =
        reinterpret_cast<const ulonglong2 *>(A.nodes + (((r * A.stride_a + 2 * A.group * A.stride_b) * polys + rest) << A.logN))[e2];
}

// zero [n_rows][2][L_in][N] (encryptions of zero, coefficient form), plain [n][N] mod t -> out [n_rows][2][L][N], n_rows = n 2 E(L)
struct BfvPlantArgs {
    const u64 *zero, *plain;
    u64 *out;
    u64 n_polys; // n_rows 2 L output residue polynomials
    u64 t;
    int L, L_in, logN;
    BfvDigitTab tab;
};

__global__ void __launch_bounds__(kBlock) k_bfv_rgsw_plant(BfvPlantArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 row = p / (2 * (u64)A.L);
    const int kk = (int)((p / (u64)A.L) & 1), ii = (int)(p % (u64)A.L);
    const BfvDigitSrc s = bfv_gadget_src(A.tab, 2, row); // row = r 2E + k E + off_i + g; s.poly = (2 r + k) L + i
    ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.zero + (((row * 2 + kk) * A.L_in + ii) << A.logN))[e2];
    if (s.prime == ii && (int)((s.poly / (u64)A.L) & 1) == kk) {
        const ModU64 mi = make_modu(primes[ii]);
        const ulonglong2 mm = reinterpret_cast<const ulonglong2 *>(A.plain + ((s.poly / (2 * (u64)A.L)) << A.logN))[e2];
        x.x = addmod(x.x, bfv_gadget_plant(mm.x, A.t, s.digit, A.tab.w, mi), mi.q);
        x.y = addmod(x.y, bfv_gadget_plant(mm.y, A.t, s.digit, A.tab.w, mi), mi.q);
    }
    reinterpret_cast<ulonglong2 *>(A.out + (p << A.logN))[e2] = x;
}

// zero [n][2][L_in][N] (encryptions of zero, coefficient form), sel [n][n_sel] mod t -> out [n][2][L][N]
struct BfvSelectorArgs {
    const u64 *zero, *sel;
    u64 *out;
    u64 n_polys; // n 2 L output residue polynomials
    u64 t, n_sel, first_slot;
    u64 inv_pow2[kMaxPrimes]; // (2^d)^(-1) mod q_i
    int L, L_in, logN;
    BfvDigitTab tab;
};

__global__ void __launch_bounds__(kBlock) k_bfv_selector_plant(BfvSelectorArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 r = p / (2 * (u64)A.L);
    const int kk = (int)((p / (u64)A.L) & 1), ii = (int)(p % (u64)A.L);
    ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.zero + (((r * 2 + kk) * A.L_in + ii) << A.logN))[e2];
    const u64 E = A.tab.total, lo = A.first_slot, hi = A.first_slot + A.n_sel * E; // the slots: coefficients lo .. hi - 1
    if (kk == 0 && 2 * e2 + 1 >= lo && 2 * e2 < hi) {
        const ModU64 mi = make_modu(primes[ii]);
        u64 xs[2] = {x.x, x.y};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u64 e = 2 * e2 + h;
            if (e < lo || e >= hi) continue;
            const u64 slot = e - lo, b = slot / E;
            const u32 d = (u32)(slot % E);
            if (bfv_digit_prime(A.tab, d) != ii) continue;
            xs[h] = addmod(xs[h], bfv_selector_value(A.sel[r * A.n_sel + b], A.t, (int)(d - A.tab.off[ii]), A.tab.w, A.inv_pow2[ii], mi), mi.q);
        }
        x = make_ulonglong2(xs[0], xs[1]);
    }
    reinterpret_cast<ulonglong2 *>(A.out + (p << A.logN))[e2] = x;
}

// s [N] under prime q0, coefficients 0, 1, q0 - 1 (in place) -> 0, 1, t - 1
__global__ void __launch_bounds__(kBlock) k_bfv_secret_plain(u64 *s, u64 n, u64 q0, u64 t)
{
    const u64 e = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const u64 x = s[e];
    s[e] = x > (q0 >> 1) ? t - (q0 - x) : x;
}

BfvGadgetCutArgs cut_args(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *in, u64 stride_a, u64 stride_b, u64 *out)
{
    if (L < 1 || L > kMaxPrimes || tab.L != L || size < 1 || size > 3 || !bfv_gadget_width_ok(tab.w))
        throw std::invalid_argument("gadget decomposition: level, size or digit table out of range");
    BfvGadgetCutArgs A{};
    A.in = in; A.out = out; A.n_b = n_b; A.stride_a = stride_a; A.stride_b = stride_b;
    A.n_polys = n_a * n_b * size * L; A.L = L; A.size = size; A.logN = env.logn1 + kRowLog; A.tab = tab;
    A.first = 0; A.own = nullptr; A.own_E = 0;
    return A;
}
template <bool OWN>
void launch_cut(const KernelEnv &env, const BfvGadgetCutArgs &A, bool cols)
{
    if (!cols) {
        hipLaunchKernelGGL(k_bfv_gadget_spread<OWN>, dim3(streaming_grid(A.n_polys, A.logN, "gadget decomposition")), dim3(kBlock), 0, env.stream, A, env.primes);
        return;
    }
    const dim3 g(grid_blocks(A.n_polys * 4, "gadget decomposition")), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL((k_bfv_gadget_cols_fwd<decltype(n1)::value, OWN>), g, b, 0, env.stream, A, env.primes); });
}

} // namespace

void launch_bfv_gadget_cut(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out, bool cols)
{
    if (!n_a || !n_b) return;
    const BfvGadgetCutArgs A = cut_args(env, tab, L, size, n_a, n_b, ct, stride_a, stride_b, out);
    if (env.logn1 == 0 && cols) throw std::invalid_argument("gadget decomposition: N = 1024 has no column pass");
    launch_cut<false>(env, A, cols);
}
void launch_bfv_gadget_cut_own(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 n_b, u64 first, u64 count, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out,
                               u64 *own, u32 own_E, bool cols)
{
    if (!count) return;
    if (!n_b || !own || !own_E) throw std::invalid_argument("he355_bfv_rgsw_from_bfv: no selectors or no output");
    BfvGadgetCutArgs A = cut_args(env, tab, L, 2, 1, count, ct, stride_a, stride_b, out); // n_polys of `count` ciphertexts
    A.n_b = n_b; A.first = first; A.own = own; A.own_E = own_E;
    if (env.logn1 == 0 && cols) throw std::invalid_argument("he355_bfv_rgsw_from_bfv: N = 1024 has no column pass");
    launch_cut<true>(env, A, cols);
}
static u64 gadget_mac_blocks(const KernelEnv &env, int L, u64 n) { return n * (u64)L * ((((u64)1 << (env.logn1 + kRowLog)) / 2) / kBlock); }
static void gadget_mac(const KernelEnv &env, int L, u64 n, u64 inner, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 rg_stride_k, u64 *out, u64 first, u32 own_E)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || inner < 1 || rows < 2 || inner * rows > 0x7fffffffull)
        throw std::invalid_argument("he355_bfv_external_product: level or inner dimension out of range");
    BfvGadgetMacArgs A{};
    A.dig = dig; A.rgsw = rgsw; A.out = out; A.n = n; A.rg_stride_r = rg_stride_r; A.rg_stride_k = rg_stride_k;
    A.inner = (u32)inner; A.rows = rows; A.L = L; A.logN = env.logn1 + kRowLog;
    A.pairs_blocks = (u32)((((u64)1 << A.logN) / 2) / kBlock);
    for (int j = 0; j < L; ++j) {
        A.run[j] = (u32)bfv_mac_run(env.prime_q[j]);
        if (A.run[j] < 2) throw std::invalid_argument("he355_bfv_external_product: prime too wide for a 128-bit sum");
    }
    const u64 blocks = gadget_mac_blocks(env, L, n);
    if (blocks > 0x7fffffffull) throw std::invalid_argument("he355_bfv_external_product: too many results for one launch");
    A.first = first; A.own_E = own_E;
    if (own_E) hipLaunchKernelGGL(k_bfv_gadget_mac<true>, dim3((unsigned)blocks), dim3(kBlock), 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL(k_bfv_gadget_mac<false>, dim3((unsigned)blocks), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bfv_gadget_mac(const KernelEnv &env, int L, u64 n, u64 inner, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 rg_stride_k, u64 *out)
{
    gadget_mac(env, L, n, inner, rows, dig, rgsw, rg_stride_r, rg_stride_k, out, 0, 0);
}
void launch_bfv_gadget_mac_own(const KernelEnv &env, int L, u64 first, u64 count, u32 rows, const u64 *dig, const u64 *key, u64 *out, u32 own_E)
{
    if (!own_E) throw std::invalid_argument("he355_bfv_rgsw_from_bfv: no selectors");
    gadget_mac(env, L, count, 1, rows, dig, key, 0, 1, out, first, own_E);
}
// ---- he355_bfv_select: one pass of one level ----------------------------------------------------------------------------------------------
void launch_bfv_select_cut(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 group, u64 first, u64 count, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, bool cols)
{
    if (!count) return;
    if (!group) throw std::invalid_argument("he355_bfv_select: a level without pairs has no cut");
    BfvGadgetCutArgs A = cut_args(env, tab, L, 2, 1, count, nodes, stride_a, stride_b, out); // n_polys of `count` pairs
    A.n_b = group; A.first = first;
    if (env.logn1 == 0 && cols) throw std::invalid_argument("he355_bfv_select: N = 1024 has no column pass");
    if (!cols) {
        hipLaunchKernelGGL(k_bfv_select_spread, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_select")), dim3(kBlock), 0, env.stream, A, env.primes);
        return;
    }
    const dim3 g(grid_blocks(A.n_polys * 4, "he355_bfv_select")), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL((k_bfv_select_cols_fwd<decltype(n1)::value>), g, b, 0, env.stream, A, env.primes); });
}
void launch_bfv_select_mac(const KernelEnv &env, int L, u64 group, u64 first, u64 count, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 *out)
{
    if (!count) return;
    if (!group || L < 1 || L > kMaxPrimes || rows < 2) throw std::invalid_argument("he355_bfv_select: level, rows or pairs out of range");
    BfvSelectMacArgs A{};
    A.dig = dig; A.rgsw = rgsw; A.out = out; A.n = count; A.rg_stride_r = rg_stride_r; A.first = first; A.group = group;
    A.rows = rows; A.L = L; A.logN = env.logn1 + kRowLog;
    A.pairs_blocks = (u32)((((u64)1 << A.logN) / 2) / kBlock);
    for (int j = 0; j < L; ++j) {
        A.run[j] = (u32)bfv_mac_run(env.prime_q[j]);
        if (A.run[j] < 2) throw std::invalid_argument("he355_bfv_select: prime too wide for a 128-bit sum");
    }
    hipLaunchKernelGGL(k_bfv_select_mac, dim3(grid_blocks(gadget_mac_blocks(env, L, count), "he355_bfv_select", "pairs")), dim3(kBlock), 0, env.stream, A, env.primes);
}
static BfvSelectTailArgs select_tail_args(const KernelEnv &env, int L, u64 group, u64 first, u64 items, const u64 *sums, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out,
                                          u64 out_stride)
{
    if (L < 1 || L > kMaxPrimes) throw std::invalid_argument("he355_bfv_select: level out of range");
    BfvSelectTailArgs A{};
    A.sums = sums; A.nodes = nodes; A.out = out; A.first = first; A.group = group; A.stride_a = stride_a; A.stride_b = stride_b; A.out_stride = out_stride;
    A.n_polys = items * 2 * L; A.L = L; A.logN = env.logn1 + kRowLog;
    return A;
}
void launch_bfv_select_tail(const KernelEnv &env, int L, u64 group, u64 first, u64 count, const u64 *sums, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, u64 out_stride)
{
    if (!count) return;
    if (!group) throw std::invalid_argument("he355_bfv_select: a level without pairs has no tail");
    const BfvSelectTailArgs A = select_tail_args(env, L, group, first, count, sums, nodes, stride_a, stride_b, out, out_stride);
    if (env.logn1 == 0) {
        hipLaunchKernelGGL(k_bfv_select_add, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_select")), dim3(kBlock), 0, env.stream, A, env.primes);
        return;
    }
    const dim3 g(grid_blocks(A.n_polys * 4, "he355_bfv_select")), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL((k_bfv_select_cols_inv<decltype(n1)::value>), g, b, 0, env.stream, A, env.primes); });
}
void launch_bfv_select_copy(const KernelEnv &env, int L, u64 n, u64 group, const u64 *nodes, u64 stride_a, u64 stride_b, u64 *out, u64 out_stride)
{
    if (!n) return;
    const BfvSelectTailArgs A = select_tail_args(env, L, group, 0, n, nullptr, nodes, stride_a, stride_b, out, out_stride);
    hipLaunchKernelGGL(k_bfv_select_copy, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_select")), dim3(kBlock), 0, env.stream, A);
}
void launch_bfv_rgsw_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, int L_in, u64 n, const u64 *zero, const u64 *plain, u64 t, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || tab.L != L || L_in < L || !bfv_gadget_width_ok(tab.w)) throw std::invalid_argument("he355_bfv_rgsw_encrypt: level or digit table out of range");
    BfvPlantArgs A{};
    A.zero = zero; A.plain = plain; A.out = out; A.n_polys = n * 2 * tab.total * 2 * L; A.t = t; A.L = L; A.L_in = L_in; A.logN = env.logn1 + kRowLog; A.tab = tab;
    hipLaunchKernelGGL(k_bfv_rgsw_plant, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_rgsw_encrypt")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bfv_selector_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, int L_in, u64 n, u64 n_sel, u64 first_slot, int d, const u64 *zero, const u64 *sel, u64 t, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || tab.L != L || L_in < L || !bfv_gadget_width_ok(tab.w) || d < 0 || d > env.logn1 + kRowLog ||
        first_slot + n_sel * tab.total > ((u64)1 << (env.logn1 + kRowLog)))
        throw std::invalid_argument("he355_bfv_selector_encrypt: level, digit table or slots out of range");
    BfvSelectorArgs A{};
    A.zero = zero; A.sel = sel; A.out = out; A.n_polys = n * 2 * L; A.t = t; A.n_sel = n_sel; A.first_slot = first_slot;
    for (int i = 0; i < L; ++i) A.inv_pow2[i] = bfv_selector_inv_pow2(env.prime_q[i], d);
    A.L = L; A.L_in = L_in; A.logN = env.logn1 + kRowLog; A.tab = tab;
    hipLaunchKernelGGL(k_bfv_selector_plant, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_selector_encrypt")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bfv_secret_plain(const KernelEnv &env, u64 *s, u64 t)
{
    const u64 N = (u64)1 << (env.logn1 + kRowLog);
    hipLaunchKernelGGL(k_bfv_secret_plain, dim3((unsigned)(N / kBlock)), dim3(kBlock), 0, env.stream, s, N, env.prime_q[0], t);
}

} // namespace HE355_KNS
} // namespace he355
