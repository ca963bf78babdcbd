// he355_kernels_bfv_level.hip -- BFV level operations on coefficient-form ciphertexts: modulus switching (Evaluator::mod_switch_to_next /
// mod_switch_to) and plaintext operands (Evaluator::add_plain, sub_plain, multiply_plain).  The per-coefficient arithmetic is
// bfv_level_core.h (host-compilable: tests/csim_bfv runs the same text on the CPU); the transforms are ntt_core.h's lane programs.
//
//   k_bfv_mod_switch     streaming; a lane owns two coefficients of one polynomial: L residues in (stride N, 16 B per access), every drop of the
//                        chain in registers, L_to residues out -- one read of L N and one write of L_to N words per polynomial however
//                        many primes go.
//   k_bfv_addsub_plain   streaming; out = ct +- Delta_L(plain) on polynomial 0, the other polynomials copied (not at all when in place).
//                        he355_encrypt's plaintext term is this kernel at the top level.
//   multiply_plain       the plaintexts of a call are lifted (k_bfv_lift_plain) and transformed once; a ciphertext polynomial then takes
//                        three launches: k_bfv_mp_cols_fwd (forward column pass, ct -> out), k_bfv_mp_rows (a wave takes its 1024-word row
//                        through the forward row pass, multiplies by the same row of the prepared plaintext and runs the inverse row pass,
//                        all in registers, in place on out) and k_cols_inv.  N = 1024 has no column pass: k_bfv_mp_rows alone, ct -> out.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_level.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

inline unsigned grid_for(u64 jobs, u64 per_block) { return (unsigned)((jobs + per_block - 1) / per_block); }

// in [n_polys][L][N] -> out [n_polys][L_to][N]; one thread = 2 coefficients of one polynomial, all its residues
template <int ML>
__global__ void __launch_bounds__(kBlock) k_bfv_mod_switch(const u64 *in, u64 *out, const PrimeDev *primes, const BfvDropConst *tab, int stride, int L, int L_to,
                                                           int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 poly = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    if (poly >= n_polys) return;
    u64 x0[ML], x1[ML];
#pragma unroll
    for (int i = 0; i < ML; ++i)
        if (i < L) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(in + ((poly * L + i) << logN))[e2];
            x0[i] = v.x; x1[i] = v.y;
        }
    bfv_drop_chain<ML>(primes, tab, stride, L, L_to, x0);
    bfv_drop_chain<ML>(primes, tab, stride, L, L_to, x1);
#pragma unroll
    for (int i = 0; i < ML; ++i)
        if (i < L_to) reinterpret_cast<ulonglong2 *>(out + ((poly * L_to + i) << logN))[e2] = make_ulonglong2(x0[i], x1[i]);
}

// out[r] = ct[ia(r)] +- (Delta_L(plain[ib(r)]), 0, ..): ct, out [.][size][L][N], plain [.][N] mod t; one thread = 2 coefficients of one result
__global__ void __launch_bounds__(kBlock) k_bfv_addsub_plain(const u64 *ct, const u64 *plain, u64 *out, Indexer ix, const PrimeDev *primes, BfvDeltaConst dc,
                                                             int L, int size, int logN, u64 n_results, int sub)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 r = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    if (r >= n_results) return;
    const u64 ctn = ((u64)size * L) << logN;
    const u64 *src = ct + idx_a(ix, r) * ctn;
    u64 *dst = out + r * ctn;
    const ulonglong2 m = reinterpret_cast<const ulonglong2 *>(plain + (idx_b(ix, r) << logN))[e2];
    const u64 fx = bfv_delta_fix(m.x, dc), fy = bfv_delta_fix(m.y, dc);
    for (int i = 0; i < L; ++i) {
        const PrimeDev &Pi = primes[i];
        const ModU64 mi = make_modu(Pi);
        const u64 dx = bfv_delta_residue(m.x, fx, dc.qdivt[i], mi), dy = bfv_delta_residue(m.y, fy, dc.qdivt[i], mi);
        const ulonglong2 c = reinterpret_cast<const ulonglong2 *>(src + ((u64)i << logN))[e2];
        ulonglong2 z;
        if (sub) { z.x = submod(c.x, dx, Pi.q); z.y = submod(c.y, dy, Pi.q); }
        else { z.x = addmod(c.x, dx, Pi.q); z.y = addmod(c.y, dy, Pi.q); }
        reinterpret_cast<ulonglong2 *>(dst + ((u64)i << logN))[e2] = z;
    }
    if (src == dst) return; // in place: the other polynomials are where they belong
    for (int p = L; p < size * L; ++p) reinterpret_cast<ulonglong2 *>(dst + ((u64)p << logN))[e2] = reinterpret_cast<const ulonglong2 *>(src + ((u64)p << logN))[e2];
}

// plain [n_plain][N] mod t -> dst [n_plain][L][N]: the centred lift under every prime of the level; one thread = 2 coefficients of one plaintext
__global__ void __launch_bounds__(kBlock) k_bfv_lift_plain(const u64 *plain, u64 *dst, const PrimeDev *primes, u64 t, int L, int logN, u64 n_plain)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 j = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    if (j >= n_plain) return;
    const ulonglong2 m = reinterpret_cast<const ulonglong2 *>(plain + (j << logN))[e2];
    for (int i = 0; i < L; ++i) {
        const ModU64 mi = make_modu(primes[i]);
        reinterpret_cast<ulonglong2 *>(dst + ((j * L + i) << logN))[e2] = make_ulonglong2(bfv_lift_centred(m.x, t, mi), bfv_lift_centred(m.y, t, mi));
    }
}

// ---- multiply_plain -----------------------------------------------------------------------------------------------------------------
// Results op_offset .. op_offset + n_ops - 1 of the batch: result r reads ciphertext ia(r) of `ct` and the prepared plaintext of ordinal
// ib(r) - b_base ([.][L][N], NTT form), and owns out[r]; all three pointers are the batch's.
struct BfvMpArgs {
    const u64 *ct, *prep;
    u64 *out;
    Indexer ix;
    u64 op_offset, n_ops;
    int L, size, logn1, pad_;
};
// forward column pass, out of place: ct[ia(r)] -> out[r] (raw of each prime).  One lane owns one stride-1024 column, as k_cols_fwd.
template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_mp_cols_fwd(BfvMpArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 pj = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int polys = A.size * A.L, p = (int)(pj % polys);
    const u64 r = A.op_offset + pj / polys;
    const u64 ctn = (u64)polys << (LOGN1 + kRowLog);
    const u64 *src = A.ct + idx_a(A.ix, r) * ctn + ((u64)p << (LOGN1 + kRowLog));
    u64 *dst = A.out + r * ctn + ((u64)p << (LOGN1 + kRowLog));
    const PrimeDev &P = primes[p % A.L];
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(src[(a << kRowLog) + col]);
        col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
    }
}
// One row of one residue polynomial of one result: forward row pass, times the plaintext's row (canonical NTT form, as k_rows_fwd stored
// it: the same lane <-> element map, slot for slot), inverse row pass.  The plaintext row is requested after the forward pass: asked for
// between its phases B and C (wave_rows_fwd_n's hook) it held 32 more registers through phase C -- 181 instead of 168 VGPRs, two waves per
// SIMD instead of three -- and measured 3 to 5 % slower (profiles/bfv_levels.txt).  `last`: N = 1024, the row is the polynomial
// (canonical in, canonical out).
template <class Ar>
__device__ __forceinline__ void bfv_mp_row(const PrimeDev &P, const u64 *src, const u64 *prow, u64 *dst, bool last, u32 rowbase, int lane, u64 *lds, bool valid)
{
    typedef typename Ar::T T;
    const Ar ar = make_ar(P, (Ar *)nullptr);
    T x[kRowE];
    u64 v[kRowE], pl[kRowE];
    load_rowA(src, lane, v);
#pragma unroll
    for (int e = 0; e < kRowE; ++e) x[e] = last ? ar.from_canon(v[e]) : ar.from_raw(v[e]);
    wave_rows_fwd(ar, tw_table(gtw(P.fwd), rowbase), lane, lds, x);
    load_rowC(prow, lane, pl);
#pragma unroll
    for (int e = 0; e < kRowE; ++e) v[e] = ar.dy_out(ar.dy_mul(ar.dy_in(ar.to_canon(x[e])), ar.dy_in(pl[e])));
#pragma unroll
    for (int e = 0; e < kRowE; ++e) x[e] = ar.from_canon(v[e]);
    wave_rows_inv(ar, P, last, rowbase, lane, lds, x);
#pragma unroll
    for (int e = 0; e < kRowE; ++e) v[e] = last ? ar.to_canon(x[e]) : ar.to_raw(x[e]);
    if (valid) store_rowA(dst, lane, v);
}
// job = (result, polynomial, residue, row); a wave owns a job, nothing is shared between the waves of a block (no workgroup barrier)
__global__ void __launch_bounds__(kBlock) k_bfv_mp_rows(BfvMpArgs A, const PrimeDev *primes, u64 total_jobs)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    u64 job = (u64)blockIdx.x * kWaves + wave;
    const bool valid = job < total_jobs;
    if (!valid) job = total_jobs - 1;
    const u32 a = (u32)(job & (n1 - 1));
    const u64 pj = job >> A.logn1;
    const int polys = A.size * A.L, p = (int)(pj % polys), i = p % A.L;
    const u64 r = A.op_offset + pj / polys;
    const bool last = A.logn1 == 0;
    const u64 ctn = (u64)polys << (A.logn1 + kRowLog);
    const u64 rowoff = ((u64)p << (A.logn1 + kRowLog)) + ((u64)a << kRowLog);
    u64 *dst = A.out + r * ctn + rowoff;
    const u64 *src = last ? A.ct + idx_a(A.ix, r) * ctn + rowoff : dst;
    const u64 *prow = A.prep + (((idx_b(A.ix, r) - A.ix.b_base) * A.L + i) << (A.logn1 + kRowLog)) + ((u64)a << kRowLog);
    const PrimeDev &P = primes[i];
    if (P.f64) bfv_mp_row<ArF64>(P, src, prow, dst, last, n1 + a, lane, lds[wave], valid);
    else bfv_mp_row<ArU64>(P, src, prow, dst, last, n1 + a, lane, lds[wave], valid);
}

} // namespace

void launch_bfv_mod_switch(const KernelEnv &env, const BfvDropConst *tab, int stride, int L, int L_to, u64 n_polys, const u64 *in, u64 *out)
{
    if (!n_polys) return;
    if (L > kBfvLevelMaxL) throw std::invalid_argument("BFV modulus switching supports up to 16 data primes");
    const int logN = env.logn1 + kRowLog;
    const dim3 g(grid_for(n_polys << (logN - 1), kBlock)), b(kBlock);
    if (L <= 4) hipLaunchKernelGGL(k_bfv_mod_switch<4>, g, b, 0, env.stream, in, out, env.primes, tab, stride, L, L_to, logN, n_polys);
    else if (L <= 8) hipLaunchKernelGGL(k_bfv_mod_switch<8>, g, b, 0, env.stream, in, out, env.primes, tab, stride, L, L_to, logN, n_polys);
    else hipLaunchKernelGGL(k_bfv_mod_switch<kBfvLevelMaxL>, g, b, 0, env.stream, in, out, env.primes, tab, stride, L, L_to, logN, n_polys);
}
void launch_bfv_addsub_plain(const KernelEnv &env, int L, int size, u64 n_results, const u64 *ct, const u64 *plain, Indexer ix, u64 *out, const BfvDeltaConst &dc,
                             bool sub)
{
    if (!n_results) return;
    const int logN = env.logn1 + kRowLog;
    hipLaunchKernelGGL(k_bfv_addsub_plain, dim3(grid_for(n_results << (logN - 1), kBlock)), dim3(kBlock), 0, env.stream, ct, plain, out, ix, env.primes, dc, L,
                       size, logN, n_results, sub ? 1 : 0);
}
void launch_bfv_lift_plain(const KernelEnv &env, int L, u64 n_plain, const u64 *plain, u64 *dst, u64 t)
{
    if (!n_plain) return;
    const int logN = env.logn1 + kRowLog;
    hipLaunchKernelGGL(k_bfv_lift_plain, dim3(grid_for(n_plain << (logN - 1), kBlock)), dim3(kBlock), 0, env.stream, plain, dst, env.primes, t, L, logN, n_plain);
}
void launch_bfv_mp_cols_fwd(const KernelEnv &env, int L, int size, u64 n_ops, u64 op_offset, const u64 *ct, Indexer ix, u64 *out)
{
    if (!n_ops || env.logn1 == 0) return;
    BfvMpArgs A{};
    A.ct = ct; A.prep = nullptr; A.out = out; A.ix = ix; A.op_offset = op_offset; A.n_ops = n_ops; A.L = L; A.size = size; A.logn1 = env.logn1;
    const unsigned g = (unsigned)(n_ops * size * L * 4);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_bfv_mp_cols_fwd<decltype(n1)::value>, dim3(g), dim3(kBlock), 0, env.stream, A, env.primes); });
}
void launch_bfv_mp_rows(const KernelEnv &env, int L, int size, u64 n_ops, u64 op_offset, const u64 *ct, const u64 *prep, Indexer ix, u64 *out)
{
    if (!n_ops) return;
    BfvMpArgs A{};
    A.ct = ct; A.prep = prep; A.out = out; A.ix = ix; A.op_offset = op_offset; A.n_ops = n_ops; A.L = L; A.size = size; A.logn1 = env.logn1;
    const u64 jobs = (n_ops * size * L) << env.logn1;
    hipLaunchKernelGGL(k_bfv_mp_rows, dim3(grid_for(jobs, kWaves)), dim3(kBlock), 0, env.stream, A, env.primes, jobs);
}

} // namespace HE355_KNS
} // namespace he355
