// he355_kernels_poly.hip -- the scalar combination of CKKS polynomial evaluation: out = sum_t a_t * ct_t + a_const with one residue per
// (term, prime) on the host side of the launch (he355_combine_scalars; the leaves of he355_ckks_eval_poly).  The per-coefficient
// arithmetic is poly_core.h (host-compilable: tests/csim/sim_poly.cpp runs the same text on the CPU).
//
//   k_scalar_combine   streaming, 16-byte accesses; a lane owns two neighbouring coefficients of one (ciphertext, polynomial, prime).
//                      One pass over the term table -- per term a pointer and a level (uniform), the scalar under the lane's prime
//                      (uniform) and 16 bytes of the term's row, read with the TERM's [L_t][N] stride, so a term at a higher level needs
//                      no drop -- into two 128-bit sums under the run rule of bfv_mac_core.h (one run length per launch: the shortest of
//                      its primes', 256 under a 60-bit prime), one reduction, one store.  All residues are u64 words in HBM in both
//                      engines: one instantiation serves fp64 and u64 primes.  Blocks are numbered ciphertext-fastest, so the blocks
//                      resident together differ in their ciphertext and share the table's words.  No LDS.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "he355_kernels.h"
#include "poly_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_poly.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

struct ScalarCombineArgs {
    const ulonglong2 *terms; // [n_terms]: {the term's slab, its level L_t}
    const u64 *scalars;      // [n_terms][L]
    const u64 *cst;          // [L], or null: no constant
    u64 *out;                // [n][size][L][N]
    u64 n;
    u64 run;                 // poly_run
    u32 n_terms;
    int L, size, logN;
};

__global__ void __launch_bounds__(kBlock) k_scalar_combine(ScalarCombineArgs A, const PrimeDev *primes)
{
    const int seg_log = A.logN - 1 - 8; // blocks per row of N / 2 pairs (kBlock = 2^8 lanes)
    const u64 b = blockIdx.x;
    const u64 c = b % A.n, rest = b / A.n;
    const u64 pi = rest >> seg_log; // (polynomial, prime)
    const int i = (int)(pi % (u64)A.L), k = (int)(pi / (u64)A.L);
    if (k >= A.size) return; // (the whole block; the grid is exact)
    const u64 e2 = ((rest & (((u64)1 << seg_log) - 1)) << 8) + threadIdx.x;
    const ModU64 m = make_modu(primes[i]);
    const u64 N = (u64)1 << A.logN;
    const u64 ck = c * (u64)A.size + (u64)k;
    u128 s0 = (k == 0 && A.cst) ? A.cst[i] : 0, s1 = s0;
    u64 left = A.run - 1;
#pragma unroll 2
    for (u32 t = 0; t < A.n_terms; ++t) {
        const ulonglong2 tm = A.terms[t]; // (uniform)
        const u64 a = A.scalars[(u64)t * (u64)A.L + (u64)i];
        const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const u64 *>(tm.x) + (ck * tm.y + (u64)i) * N)[e2];
        if (bsgs_run_full(left, A.run)) {
            bfv_mac_fold(s0, m); bfv_mac_fold(s1, m);
        }
        bfv_mac_add(s0, x.x, a); bfv_mac_add(s1, x.y, a);
        --left;
    }
    reinterpret_cast<ulonglong2 *>(A.out + (ck * (u64)A.L + (u64)i) * N)[e2] = make_ulonglong2(bfv_mac_reduce(s0, m), bfv_mac_reduce(s1, m));
}

} // namespace

void launch_scalar_combine(const KernelEnv &env, int L, int size, u64 n, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || size < 1 || size > 3 || !n_terms || n_terms > 0xffffffffull || !d_terms || !d_scalars || !out)
        throw std::runtime_error("he355_combine_scalars: the launch needs a level, a size of 1..3, between one and 2^32 - 1 terms and its tables");
    ScalarCombineArgs A{};
    A.terms = reinterpret_cast<const ulonglong2 *>(d_terms); A.scalars = d_scalars; A.cst = d_const; A.out = out;
    A.n = n; A.n_terms = (u32)n_terms; A.L = L; A.size = size; A.logN = env.logn1 + kRowLog;
    A.run = poly_run(env.prime_q, L);
    if (A.run < 2) throw std::runtime_error("he355_combine_scalars: prime too wide for a 128-bit sum");
    const u64 blocks = (n * (u64)size * (u64)L) << (A.logN - 9);
    hipLaunchKernelGGL(k_scalar_combine, dim3(grid_blocks(blocks, "he355_combine_scalars", "ciphertexts")), dim3(kBlock), 0, env.stream, A, env.primes);
}

} // namespace HE355_KNS
} // namespace he355
