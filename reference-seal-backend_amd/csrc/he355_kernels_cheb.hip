// he355_kernels_cheb.hip -- the fused combine-and-rescale step of the Chebyshev evaluation (he355_combine_scalars_rescale; every power and
// every leaf of he355_ckks_eval_chebyshev): out = rescale(sum_t a_t * ct_t + a_const) without the combined [L][N] slab.  The per-lane
// arithmetic is cheb_core.h (host-compilable: tests/csim/sim_cheb.cpp runs the same text on the CPU).
//
//   k_scalar_combine_row     k_scalar_combine's lane program (he355_kernels_poly.hip) for row L - 1 alone -- the prime the rescale divides
//                            out -- written to a compact [n size][N] block: the source of the inverse row pass (k_rows_inv_select) and the
//                            floor step's column half (k_floor_colsn), both unchanged.
//   k_floor_rows_combine<Ar> the floor step's row half (floor_rows_block of he355_kernels_ks.hip without its tail) whose source word is not
//                            loaded from a slab: a wave forms tv[r] = reduce(sum_t a_t x_t[r] + const) for its 16 elements per lane from
//                            the term rows themselves -- read through load_rowC with each TERM's [L_t][N] stride, integer sums under every
//                            prime in both engines -- then transforms the correction row and finishes with ar.floor_fin.  T row reads and
//                            one row write per (ciphertext, polynomial, prime < L - 1); the sums come first, so the 64 VGPRs of
//                            accumulators are dead before the transform starts.
// Both read the term table he355_combine_scalars uploads ({slab, level} pairs, scalars [n_terms][L], constant [L]) and take the chunk's
// first ciphertext as an argument: one table serves every chunk of a call.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "he355_kernels.h"
#include "cheb_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_cheb.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

struct CombineTable {
    const ulonglong2 *terms; // [n_terms]: {the term's slab [.][size][L_t][N], its level L_t}
    const u64 *scalars;      // [n_terms][L]
    const u64 *cst;          // [L], or null: no constant
    u64 op_off;              // the chunk's first ciphertext in the terms' slabs
    u64 run;                 // poly_run
    u32 n_terms;
    int L, size;
};

struct CombineRowArgs {
    CombineTable t;
    u64 *row; // [n][size][N]
    u64 n;
    int logN;
};

__global__ void __launch_bounds__(kBlock) k_scalar_combine_row(CombineRowArgs A, const PrimeDev *primes)
{
    const int seg_log = A.logN - 1 - 8; // blocks per row of N / 2 pairs (kBlock = 2^8 lanes)
    const u64 b = blockIdx.x;
    const u64 c = b % A.n, rest = b / A.n;
    const int k = (int)(rest >> seg_log);
    if (k >= A.t.size) return; // (the whole block; the grid is exact)
    const int i = A.t.L - 1;
    const u64 e2 = ((rest & (((u64)1 << seg_log) - 1)) << 8) + threadIdx.x;
    const ModU64 m = make_modu(primes[i]);
    const u64 N = (u64)1 << A.logN;
    const u64 ck = (A.t.op_off + c) * (u64)A.t.size + (u64)k;
    u128 s[2];
    u64 left;
    cheb_sum_open(s, (k == 0 && A.t.cst) ? A.t.cst[i] : 0, left, A.t.run);
#pragma unroll 2
    for (u32 t = 0; t < A.t.n_terms; ++t) {
        const ulonglong2 tm = A.t.terms[t]; // (uniform)
        const u64 a = A.t.scalars[(u64)t * (u64)A.t.L + (u64)i];
        const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const u64 *>(tm.x) + (ck * tm.y + (u64)i) * N)[e2];
        const u64 xv[2] = {x.x, x.y};
        cheb_sum_term(s, xv, a, left, A.t.run, m);
    }
    u64 v[2];
    cheb_sum_close(s, m, v);
    reinterpret_cast<ulonglong2 *>(A.row + (c * (u64)A.t.size + (u64)k) * N)[e2] = make_ulonglong2(v[0], v[1]);
}

struct FloorRowsCombineDev {
    CombineTable t;
    const u64 *cols; // [n_ops * size][L - 1][N] raw: launch_floor_cols(prime L - 1 -> L - 1 targets)
    u64 *out;        // [n_ops][size][L - 1][N]
    const FloorConst *fc;
    u64 n_ops;
    int K, logn1;
    int n_i;
    u32 jobs_per_block; // multiple of kWaves
    unsigned char i_list[64];
};

template <class Ar>
__global__ void __launch_bounds__(kBlock) k_floor_rows_combine(FloorRowsCombineDev A, const PrimeDev *primes)
{
    typedef typename Ar::T T;
    constexpr bool kF64 = std::is_same<Ar, ArF64>::value;
    __shared__ u64 lds[kWaves][kLdsRow];
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kF64 ? kRowTw * 8 : kRowTw * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    const int n_tgt = A.t.L - 1, src_prime = A.t.L - 1;
    // a block owns one (target prime, row) tile and walks jobs_per_block consecutive (op, poly) jobs of it, one job per wave per step
    const u64 n_jobs = A.n_ops * (u64)A.t.size;
    const u64 n_jb = (n_jobs + A.jobs_per_block - 1) / A.jobs_per_block;
    const u64 tile = blockIdx.x / n_jb;
    const u64 j_begin = (blockIdx.x % n_jb) * A.jobs_per_block;
    const u64 j_end = j_begin + A.jobs_per_block < n_jobs ? j_begin + A.jobs_per_block : n_jobs;
    const int i = A.i_list[tile >> A.logn1];
    const u32 a_row = (u32)(tile & (n1 - 1));
    const PrimeDev &P = primes[i];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const ModU64 m = make_modu(P);
    const FloorConst fc = A.fc[src_prime * A.K + i];
    const u64 rowoff = (u64)a_row << kRowLog;
    const auto twr = stage_row_twiddles<Ar, kBlock>(P, ar, n1 + a_row, twl_raw);
    __syncthreads();
    for (u64 j = j_begin + wave; j < j_end; j += kWaves) { // no block-level synchronisation inside: waves run independently
        const int k = (int)(j % (u64)A.t.size);
        const u64 op = j / (u64)A.t.size;
        u64 tv[kRowE];
        {
            u128 s[kRowE];
            u64 left;
            cheb_sum_open(s, (k == 0 && A.t.cst) ? A.t.cst[i] : 0, left, A.t.run);
            const u64 ck = (A.t.op_off + op) * (u64)A.t.size + (u64)k;
#pragma unroll 1
            for (u32 t = 0; t < A.t.n_terms; ++t) {
                const ulonglong2 tm = A.t.terms[t]; // (uniform)
                const u64 a = A.t.scalars[(u64)t * (u64)A.t.L + (u64)i];
                u64 xv[kRowE];
                load_rowC(reinterpret_cast<const u64 *>(tm.x) + (ck * tm.y + (u64)i) * N + rowoff, lane, xv);
                cheb_sum_term(s, xv, a, left, A.t.run, m);
            }
            cheb_sum_close(s, m, tv);
        }
        T x[kRowE];
        u64 v[kRowE];
        load_rowA(A.cols + ((op * (u64)A.t.size + (u64)k) * (u64)n_tgt + (u64)i) * N + rowoff, lane, v);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) x[r] = ar.from_raw(v[r]);
        wave_rows_fwd(ar, twr, lane, lds[wave], x);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = cheb_floor(ar, tv[r], x[r], fc);
        store_rowC(A.out + ((op * (u64)A.t.size + (u64)k) * (u64)n_tgt + (u64)i) * N + rowoff, lane, v);
    }
}

CombineTable combine_table(const KernelEnv &env, const char *what, int L, int size, u64 op_off, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const)
{
    if (L < 2 || L > kMaxPrimes || size < 1 || size > 3 || !n_terms || n_terms > 0xffffffffull || !d_terms || !d_scalars)
        throw std::runtime_error(std::string(what) + ": the launch needs a level of at least 2, a size of 1..3, between one and 2^32 - 1 terms and its tables");
    CombineTable t{};
    t.terms = reinterpret_cast<const ulonglong2 *>(d_terms); t.scalars = d_scalars; t.cst = d_const;
    t.op_off = op_off; t.n_terms = (u32)n_terms; t.L = L; t.size = size;
    t.run = poly_run(env.prime_q, L);
    if (t.run < 2) throw std::runtime_error(std::string(what) + ": prime too wide for a 128-bit sum");
    return t;
}

} // namespace

void launch_scalar_combine_row(const KernelEnv &env, int L, int size, u64 n, u64 op_off, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *row)
{
    if (!n) return;
    CombineRowArgs A{};
    A.t = combine_table(env, "he355_combine_scalars_rescale", L, size, op_off, d_terms, n_terms, d_scalars, d_const);
    if (!row) throw std::runtime_error("he355_combine_scalars_rescale: the row launch needs its block");
    A.row = row; A.n = n; A.logN = env.logn1 + kRowLog;
    const u64 blocks = (n * (u64)size) << (A.logN - 9);
    hipLaunchKernelGGL(k_scalar_combine_row, dim3(grid_blocks(blocks, "he355_combine_scalars_rescale", "ciphertexts")), dim3(kBlock), 0, env.stream, A, env.primes);
}

void launch_floor_rows_combine(const KernelEnv &env, int L, int size, u64 n, u64 op_off, const u64 *cols, const void *d_terms, u64 n_terms, const u64 *d_scalars,
                               const u64 *d_const, u64 *out)
{
    if (!n) return;
    FloorRowsCombineDev A{};
    A.t = combine_table(env, "he355_combine_scalars_rescale", L, size, op_off, d_terms, n_terms, d_scalars, d_const);
    if (!cols || !out) throw std::runtime_error("he355_combine_scalars_rescale: the floor launch needs its corrections and its output");
    A.cols = cols; A.out = out; A.fc = env.floor_consts; A.n_ops = n; A.K = env.K; A.logn1 = env.logn1;
    const FloorRowsGeometry G = floor_rows_geometry(ks_launch_dims(env), n, L - 1, size, -1);
    A.jobs_per_block = G.jobs_per_block;
    const u64 n_jb = (n * (u64)size + G.jobs_per_block - 1) / G.jobs_per_block;
    for (int pass = 0; pass < 4; pass += 2) { // the fp64 engine's targets, then the u64 engine's (no tail prime: passes 1 and 3 are empty)
        if (!G.i_list[pass].n) continue;
        copy_list(A.i_list, A.n_i, G.i_list[pass]);
        const unsigned g = grid_blocks((((u64)A.n_i) << env.logn1) * n_jb, "he355_combine_scalars_rescale", "ciphertexts");
        if (pass == 0) hipLaunchKernelGGL((k_floor_rows_combine<ArF64>), dim3(g), dim3(kBlock), 0, env.stream, A, env.primes);
        else hipLaunchKernelGGL((k_floor_rows_combine<ArU64>), dim3(g), dim3(kBlock), 0, env.stream, A, env.primes);
    }
}

} // namespace HE355_KNS
} // namespace he355
