// he355_kernels_behz.hip -- the BFV ct x ct multiply in the BEHZ RNS form (per-coefficient arithmetic: behz_core.h, host-compilable) and
// the coefficient-form ends of a BFV key switch.
//
//   k_behz_extend, k_behz_extend_cols       steps (1)-(2): base extension to Bsk, alone or with the forward column passes in its epilogue
//   k_behz_rows_tensor, k_behz_tensor_inv   steps (3)-(5) on rows: transforms, dyadic tensor, inverse row pass (and their _dual forms)
//   k_behz_floor_sk, k_behz_cols_floor_sk   steps (6)-(8): fast floor and Shenoy-Kumaresan, alone or behind the inverse column passes
//   k_bfv_galois                            coefficient-form automorphism as a gather
//   k_bfv_tail_sp, k_bfv_tail_fin           the key switch's mod-down in coefficient form
//
// Which route a multiply takes (behz_cols_fusable and what the launchers return): tests/bfv_multiply_plan.py restates it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <type_traits>

#include "he355_kernels.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_behz.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// =======================================================================================================
// BFV: BEHZ base extension / floor kernels (one lane = one coefficient across all residues), coefficient-form Galois,
// and the coefficient-form key-switch tails
// =======================================================================================================
__device__ __forceinline__ ModU64 mod_of(const PrimeDev *primes, int idx) { return make_modu(primes[idx]); }

// ML / MB: compile-time bounds of the bases q and B (loops fully unrolled under them, per-residue values in registers): <4, 6> serves
// the reference's default parameter sets ({60,40,40} and {60,40,40,40}), <kBehzMaxL, kBehzMaxB> everything else.
template <int ML, int MB>
__global__ void __launch_bounds__(kBlock) k_behz_extend(BehzDev Z, const PrimeDev *primes, BehzSrc src_of, u64 *xq, u64 *xbsk, u64 n_polys, int logN)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 n = gid & (((u64)1 << logN) - 1);
    const u64 pid = gid >> logN; // (ciphertext item, which poly)
    if (pid >= n_polys) return;
    const int k = (int)(pid & 1);
    constexpr int kUnrollB = MB <= 6 ? MB + 1 : 1; // the small instantiation unrolls its residue loops, the large one keeps them rolled
    const int L = Z.L, S = Z.nB + 1;
    const u64 N = (u64)1 << logN, P1 = (u64)L * N;
    const u64 *src = behz_src_ct(src_of, pid >> 1, 2 * P1) + (u64)k * P1 + n;
    u64 x[ML], tmp[ML], rmt;
#pragma unroll
    for (int i = 0; i < ML; ++i)
        if (i < L) {
            x[i] = src[(u64)i * N];
            xq[(pid * L + i) * N + n] = x[i];
        }
    behz_ext_prepare<ML>(Z, primes, L, x, tmp, rmt);
#pragma unroll kUnrollB
    for (int j = 0; j < MB + 1; ++j) {
        if (j >= S) break;
        xbsk[(pid * S + j) * N + n] = behz_ext_residue<ML>(Z, mod_of(primes, Z.bsk_prime[j]), L, j, tmp, rmt);
    }
}

// Forward column pass of one residue's column held in registers (canonical in, raw out), by the engine that owns the prime.
template <int LOGN1> __device__ __forceinline__ void col_fwd_store(const PrimeDev &P, const u64 v[1 << LOGN1], u64 *dst)
{
    constexpr int N1 = 1 << LOGN1;
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double y[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) y[a] = ar.from_canon(v[a]);
        col_fwd<ArF64, LOGN1>(ar, y, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[a << kRowLog] = ar.to_raw(y[a]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 y[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) y[a] = v[a];
        col_fwd<ArU64, LOGN1>(ar, y, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) dst[a << kRowLog] = y[a];
    }
}
// BEHZ steps (1)-(2) AND the forward column pass of all L + S residues in one kernel (N <= 16384, L <= 4, nB <= 6), so that the
// coefficient-form copies xq / xbsk never exist in HBM (k_behz_extend + k_cols_fwd x2 write them and read them back: 2 (L + S)
// polynomial transfers per input polynomial saved).  A block = 64 columns x N1 rows of one input polynomial, one wave per row:
// phase 1, lane (row e, column c) extends its coefficient to Bsk and parks the L + S residues in LDS [residue][e][c]; phase 2, wave w
// takes residues w, w + N1, ...: each lane runs that residue's column pass on the N1 values of its column (wave-uniform prime, so
// the engine branch does not diverge) and stores the raw rows.
template <int LOGN1, int ML, int MB, bool EXACT>
__global__ void __launch_bounds__(64 << LOGN1) k_behz_extend_cols(BehzDev Z, const PrimeDev *primes, BehzSrc src_of, u64 *xq, u64 *xbsk)
{
    constexpr int N1 = 1 << LOGN1;
    extern __shared__ u64 behz_sm[]; // [L + S][N1][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 pid = blockIdx.x >> 4; // (ciphertext item, which poly); 16 column groups per polynomial
    const u64 col = ((blockIdx.x & 15) << 6) | lane;
    const int k = (int)(pid & 1);
    const int L = EXACT ? ML : Z.L, S = (EXACT ? MB : Z.nB) + 1;
    const u64 N = (u64)N1 << kRowLog, P1 = (u64)L * N;
    {
        const u64 *src = behz_src_ct(src_of, pid >> 1, 2 * P1) + (u64)k * P1 + ((u64)wave << kRowLog) + col;
        u64 x[ML], tmp[ML], rmt;
#pragma unroll
        for (int i = 0; i < ML; ++i)
            if (i < L) {
                x[i] = src[(u64)i * N];
                behz_sm[((i * N1 + wave) << 6) | lane] = x[i];
            }
        behz_ext_prepare<ML>(Z, primes, L, x, tmp, rmt);
#pragma unroll
        for (int j = 0; j < MB + 1; ++j) {
            if (j >= S) break;
            behz_sm[(((L + j) * N1 + wave) << 6) | lane] = behz_ext_residue<ML>(Z, mod_of(primes, Z.bsk_prime[j]), L, j, tmp, rmt);
        }
    }
    __syncthreads();
    for (int rr = wave; rr < L + S; rr += N1) {
        const bool isq = rr < L;
        const PrimeDev &P = primes[isq ? rr : Z.bsk_prime[rr - L]];
        u64 *dst = (isq ? xq + (pid * L + rr) * N : xbsk + (pid * S + (rr - L)) * N) + col;
        u64 v[N1];
#pragma unroll
        for (int e = 0; e < N1; ++e) v[e] = behz_sm[((rr * N1 + e) << 6) | lane];
        col_fwd_store<LOGN1>(P, v, dst);
    }
}

// BEHZ steps (3)-(5) on rows: forward row pass of the four polynomials a0, a1, b0, b1 of one (op, residue, row), the dyadic tensor
// c0 = a0 b0, c1 = a0 b1 + a1 b0, c2 = a1 b1, and the inverse row pass of the three products, in ONE kernel: a block is four waves,
// wave w transforms polynomial w's row; the canonical NTT-form rows meet in LDS (each wave's own exchange buffer, free once its
// transform is done; every wave uses the same lane <-> element map, so the hand-over is slot-for-slot); waves 0..2 form one product
// each and run its inverse row pass.  Replaces k_rows_fwd (4 polynomials) + k_tensor4 + k_rows_inv (3 polynomials): 35 instead of 105
// polynomial transfers through HBM per (op, residue).  x [n*4][Lx][N] after the forward column pass (raw; canonical when N = 1024),
// d [n*3][Lx][N] ready for the inverse column pass.
struct BehzRowsArgs {
    const u64 *x[2]; // base q, base Bsk: [n*4][Lx][N]
    u64 *d[2];       //                   [n*3][Lx][N]
    int Lx[2];
    u64 n_ops;
    int logn1, n_r;
    unsigned char r_base[64], r_idx[64], r_prime[64]; // the residues of one arithmetic engine: base, index in it, device prime
};
// (body as a device function: k_behz_rows_tensor_dual runs the blocks of both engines in one launch when the grids are small)
template <class Ar>
__device__ __forceinline__ void behz_rows_tensor_block(const BehzRowsArgs &A, const PrimeDev *primes, const u64 job, u64 (*lds)[kLdsRow])
{
    typedef typename Ar::T T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    const u32 a_row = (u32)(job & (n1 - 1)); // job = (op, residue slot, row)
    const u64 orr = job >> A.logn1;
    const int slot = (int)(orr % A.n_r);
    const u64 op = orr / A.n_r;
    const int base = A.r_base[slot], r = A.r_idx[slot], Lx = A.Lx[base];
    const PrimeDev &P = primes[A.r_prime[slot]];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const bool last = A.logn1 == 0;
    const u64 rowoff = ((u64)r << (A.logn1 + kRowLog)) + ((u64)a_row << kRowLog);
    const u64 *xin = A.x[base];
    u64 *dout = A.d[base];
    // phase 1: this wave's polynomial through the forward row pass; canonical values parked in its exchange buffer
    {
        T x[kRowE];
        u64 v[kRowE];
        load_rowA(xin + (op * 4 + wave) * Lx * N + rowoff, lane, v);
#pragma unroll
        for (int e = 0; e < kRowE; ++e) x[e] = last ? ar.from_canon(v[e]) : ar.from_raw(v[e]);
        wave_rows_fwd(ar, tw_table(gtw(P.fwd), n1 + a_row), lane, lds[wave], x);
#pragma unroll
        for (int e = 0; e < kRowE; ++e) lds[wave][(e << 6) | lane] = ar.to_canon(x[e]);
    }
    __syncthreads();
    // phase 2: one product per wave (waves 0..2), from the rows the other waves parked (slot-for-slot: same lane, same register)
    const bool worker = wave < 3; // wave-uniform; wave 3 only keeps the barriers company
    u64 c[kRowE];
    if (worker) {
        u64 p0[kRowE], p1[kRowE];
        const int ia = wave == 2 ? 1 : 0, ib = wave == 0 ? 2 : 3; // c0: a0 b0; c1: a0 b1 (+ a1 b0); c2: a1 b1
#pragma unroll
        for (int e = 0; e < kRowE; ++e) { p0[e] = lds[ia][(e << 6) | lane]; p1[e] = lds[ib][(e << 6) | lane]; }
        if (wave == 1) {
            u64 q0[kRowE], q1[kRowE];
#pragma unroll
            for (int e = 0; e < kRowE; ++e) { q0[e] = lds[1][(e << 6) | lane]; q1[e] = lds[2][(e << 6) | lane]; }
#pragma unroll
            for (int e = 0; e < kRowE; ++e)
                c[e] = ar.dy_out(ar.dy_add(ar.dy_mul(ar.dy_in(p0[e]), ar.dy_in(p1[e])), ar.dy_mul(ar.dy_in(q0[e]), ar.dy_in(q1[e]))));
        } else {
#pragma unroll
            for (int e = 0; e < kRowE; ++e) c[e] = ar.dy_out(ar.dy_mul(ar.dy_in(p0[e]), ar.dy_in(p1[e])));
        }
    }
    __syncthreads(); // every wave has read what it needs before any exchange buffer is written again
    if (!worker) return;
    T x[kRowE];
#pragma unroll
    for (int e = 0; e < kRowE; ++e) x[e] = ar.from_canon(c[e]);
    wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
    u64 v[kRowE];
#pragma unroll
    for (int e = 0; e < kRowE; ++e) v[e] = last ? ar.to_canon(x[e]) : ar.to_raw(x[e]);
    store_rowA(dout + (op * 3 + wave) * Lx * N + rowoff, lane, v);
}
template <class Ar>
__global__ void __launch_bounds__(kBlock) k_behz_rows_tensor(BehzRowsArgs A, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    behz_rows_tensor_block<Ar>(A, primes, blockIdx.x, lds);
}
__global__ void __launch_bounds__(kBlock) k_behz_rows_tensor_dual(BehzRowsArgs AF, BehzRowsArgs AU, unsigned n_f, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    if (blockIdx.x < n_f) behz_rows_tensor_block<ArF64>(AF, primes, blockIdx.x, lds);
    else behz_rows_tensor_block<ArU64>(AU, primes, blockIdx.x - n_f, lds);
}

// BEHZ steps (4)-(5) when the operands were transformed once each (BehzSrc lists: he355_api.hip, bfv_multiply3): one WAVE per
// (result, residue, row, product k): it reads the canonical NTT-form rows of its operands where the one-off transform left them
// (layout C, as k_rows_fwd stores them), forms c0 = a0 b0, c1 = a0 b1 + a1 b0 or c2 = a1 b1 and runs the inverse row pass.  No
// barrier, no LDS hand-over; an operand row read by many results comes from L2 / MALL.  e [(ordinal * 2 + poly)][Lx][N],
// d [(r * 3 + k)][Lx][N] ready for the inverse column pass.
struct BehzTensorArgs {
    const u64 *e[2]; // base q, base Bsk
    u64 *d[2];
    int Lx[2];
    BehzSrc src;     // result -> operand ordinals
    u64 n_ops, op_offset;
    int logn1, n_r;
    unsigned char r_base[64], r_idx[64], r_prime[64];
};
template <class Ar>
__device__ __forceinline__ void behz_tensor_inv_block(const BehzTensorArgs &A, const PrimeDev *primes, const u64 total_jobs, const unsigned bid_x,
                                                      u64 (*lds)[kLdsRow])
{
    typedef typename Ar::T T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 job = (u64)bid_x * kWaves + wave; // (op, residue slot, row, k)
    if (job >= total_jobs) return;              // (waves are independent: no barrier below)
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    const int k = (int)(job % 3);
    const u64 j1 = job / 3;
    const u32 a_row = (u32)(j1 & (n1 - 1));
    const u64 orr = j1 >> A.logn1;
    const int slot = (int)(orr % A.n_r);
    const u64 op = orr / A.n_r;
    const int base = A.r_base[slot], r = A.r_idx[slot], Lx = A.Lx[base];
    const PrimeDev &P = primes[A.r_prime[slot]];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const bool last = A.logn1 == 0;
    const u64 rowoff = ((u64)r << (A.logn1 + kRowLog)) + ((u64)a_row << kRowLog);
    const u64 oa = ord_a(A.src, A.op_offset + op), ob = ord_b(A.src, A.op_offset + op);
    const u64 *ea = A.e[base] + oa * 2 * Lx * N + rowoff, *eb = A.e[base] + ob * 2 * Lx * N + rowoff;
    const u64 P1 = (u64)Lx * N;
    T x[kRowE];
    {
        u64 p0[kRowE], p1[kRowE];
        load_rowC(ea + (k == 2 ? P1 : 0), lane, p0); // c0: a0 b0; c1: a0 b1 (+ a1 b0); c2: a1 b1
        load_rowC(eb + (k == 0 ? 0 : P1), lane, p1);
        if (k == 1) {
            u64 q0[kRowE], q1[kRowE];
            load_rowC(ea + P1, lane, q0);
            load_rowC(eb, lane, q1);
#pragma unroll
            for (int e = 0; e < kRowE; ++e)
                x[e] = ar.from_canon(ar.dy_out(ar.dy_add(ar.dy_mul(ar.dy_in(p0[e]), ar.dy_in(p1[e])), ar.dy_mul(ar.dy_in(q0[e]), ar.dy_in(q1[e])))));
        } else {
#pragma unroll
            for (int e = 0; e < kRowE; ++e) x[e] = ar.from_canon(ar.dy_out(ar.dy_mul(ar.dy_in(p0[e]), ar.dy_in(p1[e]))));
        }
    }
    wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
    u64 v[kRowE];
#pragma unroll
    for (int e = 0; e < kRowE; ++e) v[e] = last ? ar.to_canon(x[e]) : ar.to_raw(x[e]);
    store_rowA(A.d[base] + (op * 3 + k) * Lx * N + rowoff, lane, v);
}
template <class Ar>
__global__ void __launch_bounds__(kBlock) k_behz_tensor_inv(BehzTensorArgs A, const PrimeDev *primes, u64 total_jobs)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    behz_tensor_inv_block<Ar>(A, primes, total_jobs, blockIdx.x, lds);
}
__global__ void __launch_bounds__(kBlock) k_behz_tensor_inv_dual(BehzTensorArgs AF, BehzTensorArgs AU, u64 jobs_f, u64 jobs_u, unsigned n_f, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    if (blockIdx.x < n_f) behz_tensor_inv_block<ArF64>(AF, primes, jobs_f, blockIdx.x, lds);
    else behz_tensor_inv_block<ArU64>(AU, primes, jobs_u, blockIdx.x - n_f, lds);
}

template <int ML, int MB>
__global__ void __launch_bounds__(kBlock) k_behz_floor_sk(BehzDev Z, const PrimeDev *primes, const u64 *dq, const u64 *ds, u64 *out, u64 n_polys, int logN)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 n = gid & (((u64)1 << logN) - 1);
    const u64 pid = gid >> logN; // (op, k)
    if (pid >= n_polys) return;
    constexpr int kUnrollB = MB <= 6 ? MB + 1 : 1, kUnrollL = ML <= 4 ? ML : 1;
    const int L = Z.L, S = Z.nB + 1;
    const u64 N = (u64)1 << logN;
    u64 vq[ML], vs[MB + 1], res[ML];
#pragma unroll kUnrollL
    for (int i = 0; i < ML; ++i)
        if (i < L) vq[i] = dq[(pid * L + i) * N + n];
#pragma unroll kUnrollB
    for (int j = 0; j < MB + 1; ++j)
        if (j < S) vs[j] = ds[(pid * S + j) * N + n];
    if (Z.f64aux) behz_floor_sk_coeff_f64<ML, MB>(Z, primes, L, Z.nB, vq, vs, res);
    else behz_floor_sk_coeff<ML, MB>(Z, primes, L, Z.nB, vq, vs, res);
#pragma unroll kUnrollL
    for (int j = 0; j < ML; ++j)
        if (j < L) out[(pid * L + j) * N + n] = res[j];
}

// Inverse column pass of one residue's column (raw in, canonical out, in registers), by the engine that owns the prime.
template <int LOGN1> __device__ __forceinline__ void col_inv_load(const PrimeDev &P, const u64 *src, u64 v[1 << LOGN1])
{
    constexpr int N1 = 1 << LOGN1;
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double y[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) y[a] = ar.from_raw(src[a << kRowLog]);
        col_inv<ArF64, LOGN1>(ar, y, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) v[a] = ar.to_canon(y[a]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 y[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) y[a] = src[a << kRowLog];
        col_inv<ArU64, LOGN1>(ar, y, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) v[a] = ar.to_canon(y[a]);
    }
}
// The inverse column pass of all L + S residues AND BEHZ steps (6)-(8) in one kernel (N <= 16384, L <= 4, nB <= 6): the mirror image of
// k_behz_extend_cols -- phase 1, wave w runs the column passes of residues w, w + N1, ... for the block's 64 columns and parks the
// canonical values in LDS [residue][e][c]; phase 2, lane (row e, column c) takes its coefficient's L + S residues through the fast
// floor and the Shenoy-Kumaresan conversion.  The coefficient-form products never exist in HBM.
// EXACT: L == ML and nB == MB (the reference's own parameter sets: {60,40}, {60,40,40}, {60,40,40,40} with as many auxiliary primes):
// every residue loop has a compile-time trip count -- straight-line code, no guards.
template <int LOGN1, int ML, int MB, bool EXACT>
__global__ void __launch_bounds__(64 << LOGN1) k_behz_cols_floor_sk(BehzDev Z, const PrimeDev *primes, const u64 *dq, const u64 *ds, u64 *out)
{
    constexpr int N1 = 1 << LOGN1;
    extern __shared__ u64 behz_sm[]; // [L + S][N1][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 pid = blockIdx.x >> 4; // (op, k)
    const u64 col = ((blockIdx.x & 15) << 6) | lane;
    const int L = EXACT ? ML : Z.L, nB = EXACT ? MB : Z.nB, S = nB + 1;
    const u64 N = (u64)N1 << kRowLog;
    for (int rr = wave; rr < L + S; rr += N1) {
        const bool isq = rr < L;
        const PrimeDev &P = primes[isq ? rr : Z.bsk_prime[rr - L]];
        const u64 *src = (isq ? dq + (pid * L + rr) * N : ds + (pid * S + (rr - L)) * N) + col;
        u64 v[N1];
        col_inv_load<LOGN1>(P, src, v);
#pragma unroll
        for (int e = 0; e < N1; ++e) behz_sm[((rr * N1 + e) << 6) | lane] = v[e];
    }
    __syncthreads();
    u64 vq[ML], vs[MB + 1], res[ML];
#pragma unroll
    for (int i = 0; i < ML; ++i)
        if (i < L) vq[i] = behz_sm[((i * N1 + wave) << 6) | lane];
#pragma unroll
    for (int j = 0; j < MB + 1; ++j)
        if (j < S) vs[j] = behz_sm[(((L + j) * N1 + wave) << 6) | lane];
    if (Z.f64aux) behz_floor_sk_coeff_f64<ML, MB>(Z, primes, L, nB, vq, vs, res);
    else behz_floor_sk_coeff<ML, MB>(Z, primes, L, nB, vq, vs, res);
#pragma unroll
    for (int j = 0; j < ML; ++j)
        if (j < L) out[(pid * L + j) * N + ((u64)wave << kRowLog) + col] = res[j];
}

// coefficient-form automorphism as a gather (2 polys of a size-2 ciphertext)
__global__ void __launch_bounds__(kBlock) k_bfv_galois(const u64 *in, const uint32_t *gather, u64 *c01, u64 c01_item_stride, u64 *tgt,
                                                       const PrimeDev *primes, int L, int logN, u64 n_ops, const u64 *addend)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 o = gid & (((u64)1 << logN) - 1);
    const u64 oi = gid >> logN;
    const u64 op = oi / L;
    if (op >= n_ops) return;
    const int i = (int)(oi % L);
    const u64 N = (u64)1 << logN, P1 = (u64)L * N;
    const u64 q = primes[i].q;
    const uint32_t g = gather[o];
    const u64 src = g & 0x7FFFFFFFu;
    const u64 *p0 = in + op * 2 * P1 + (u64)i * N;
    u64 v0 = p0[src], v1 = p0[P1 + src];
    if (g >> 31) { v0 = v0 ? q - v0 : 0; v1 = v1 ? q - v1 : 0; }
    u64 *o0 = c01 + op * c01_item_stride + (u64)i * N + o;
    u64 w1 = 0;
    if (addend) { // out = addend + rotate(in)
        const u64 *ad = addend + op * 2 * P1 + (u64)i * N + o;
        v0 = addmod(v0, ad[0], q);
        w1 = ad[P1];
    }
    o0[0] = v0;
    o0[P1] = w1;
    tgt[(op * L + i) * N + o] = v1;
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_tail_sp(const u64 *tpr, u64 *rp, const PrimeDev *primes, int sp)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    const u64 poly = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const u64 *src = tpr + poly * N;
    const PrimeDev &Ps = primes[sp];
    u64 c[N1];
    if (LOGN1 == 0) {
        c[0] = src[col];
    } else if (Ps.f64) {
        const ArF64 ar = make_ar(Ps, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(Ps.inv), Ps.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    } else {
        const ArU64 ar = make_ar(Ps, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(Ps.inv), Ps.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    }
    const u64 half = Ps.q >> 1;
#pragma unroll
    for (int a = 0; a < N1; ++a) rp[poly * N + (a << kRowLog) + col] = addmod(c[a], half, Ps.q);
}

// k_bfv_tail_fin is memory-bound and latency-hidden by occupancy alone: at 101 registers five waves fit a SIMD, and the 6144 waves of
// BASELINE configs[4]'s calls (64 ciphertexts x 2 x 3 polynomials) ran as one full round plus a fifth of one.  Held to six waves per SIMD
// (80 registers, 32 spilled) the call is one round: 109 -> 95 us, the matrix product 67.1 -> 65.3 ms.
template <int LOGN1>
__global__ void __launch_bounds__(kBlock, 6) k_bfv_tail_fin(const u64 *t, const u64 *rp, u64 *c01, u64 c01_item_stride, const u64 *add01,
                                                            u64 add01_item_stride, const PrimeDev *primes, const FloorConst *fcs, int L, int K)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    const u64 pid = blockIdx.x >> 2; // (op, k, i)
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int i = (int)(pid % L);
    const u64 ok = pid / L;
    const int k = (int)(ok & 1);
    const u64 op = ok >> 1;
    const u64 *src = t + pid * N;
    const PrimeDev &Pi = primes[i];
    const PrimeDev &Ps = primes[K - 1];
    u64 c[N1];
    if (LOGN1 == 0) {
        c[0] = src[col];
    } else if (Pi.f64) {
        const ArF64 ar = make_ar(Pi, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(Pi.inv), Pi.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    } else {
        const ArU64 ar = make_ar(Pi, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(Pi.inv), Pi.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    }
    const FloorConst fc = fcs[(K - 1) * K + i];
    const ModU64 mi = make_modu(Pi);
    const u64 qi = Pi.q, qs = Ps.q;
    u64 *dst = c01 + op * c01_item_stride + ((u64)k * L + i) * N;
    const u64 *add = add01 + op * add01_item_stride + ((u64)k * L + i) * N; // what the key-switched part is added to (may be dst itself)
#pragma unroll
    for (int a = 0; a < N1; ++a) {
        const u64 r = rp[ok * N + (a << kRowLog) + col];
        const u64 delta = submod(qs > qi ? barrett64(r, mi) : r, fc.half_mod, qi);
        const u64 res = mulmod(submod(c[a], delta, qi), fc.inv, mi); // (a prime of either engine: Barrett)
        const u64 idx = (a << kRowLog) + col;
        dst[idx] = addmod(add[idx], res, qi);
    }
}

} // namespace

// =======================================================================================================
// Launchers
// =======================================================================================================
bool launch_behz_extend(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_cts, u64 *xq, u64 *xbsk)
{
    const bool wide = !(bz.L <= 4 && bz.nB <= 6);
    if (!n_cts) return wide;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_cts * 2) << logN;
    if (!wide)
        hipLaunchKernelGGL((k_behz_extend<4, 6>), dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, bz, env.primes, src, xq, xbsk, n_cts * 2, logN);
    else
        hipLaunchKernelGGL((k_behz_extend<kBehzMaxL, kBehzMaxB>), dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, bz, env.primes, src, xq, xbsk, n_cts * 2, logN);
    return wide;
}
// The dynamic LDS one block of the fused column kernels may ask for on the current device, queried once per device (and per build of the
// device code: a function's attributes belong to the device it was loaded on, he355_kernels_lds.hip).  The LOGN1 = 4 pair is the only one
// that can pass 64 KiB (up to 4 + 7 residues of 8 KiB = 88 KiB): where the device reports more than 64 KiB per block, both kernels are
// opted in here to what they can ask for, and a refusal leaves the limit at 64 KiB -- behz_cols_fusable then sends the larger shapes
// down the unfused route instead of into a launch the runtime would refuse.
constexpr size_t kBehzColsLdsNoOptIn = 64u << 10, kBehzColsLdsMax4 = (size_t)(4 + 6 + 1) * (64u << 4) * 8;
size_t behz_cols_lds_limit(const KernelEnv &)
{
    static size_t limit_dev[64] = {}; // 0: not asked yet
    int dev_id = 0;
    if (hipGetDevice(&dev_id) != hipSuccess || dev_id < 0 || dev_id >= 64) dev_id = 63; // (slot 63 is never kept: asked every time)
    if (limit_dev[dev_id]) return limit_dev[dev_id];
    int per_block = 0, optin = 0;
    if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev_id == 63 ? 0 : dev_id) != hipSuccess || per_block <= 0) {
        (void)hipGetLastError();
        per_block = (int)kBehzColsLdsNoOptIn;
    }
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev_id == 63 ? 0 : dev_id) != hipSuccess) {
        (void)hipGetLastError(); // (a runtime without the attribute: the plain limit stands)
        optin = 0;
    }
    size_t limit = (size_t)std::max(per_block, optin);
    if (limit > kBehzColsLdsNoOptIn) {
        const int want = (int)std::min(limit, kBehzColsLdsMax4);
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_behz_extend_cols<4, 4, 6, false>), hipFuncAttributeMaxDynamicSharedMemorySize, want) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(&k_behz_cols_floor_sk<4, 4, 6, false>), hipFuncAttributeMaxDynamicSharedMemorySize, want) != hipSuccess) {
            (void)hipGetLastError();
            limit = kBehzColsLdsNoOptIn;
        }
    }
    if (dev_id != 63) limit_dev[dev_id] = limit;
    return limit;
}
size_t behz_cols_lds_bytes(const KernelEnv &env, const BehzDev &bz) { return (size_t)(bz.L + bz.nB + 1) * (64u << env.logn1) * 8; }
// a pure function of (N, L, nB, the device's limit): tests/bfv_multiply_plan.py restates it
bool behz_cols_fusable(const KernelEnv &env, const BehzDev &bz)
{
    return bz.L <= 4 && bz.nB <= 6 && env.logn1 >= 1 && env.logn1 <= 4 && behz_cols_lds_bytes(env, bz) <= behz_cols_lds_limit(env);
}
// The fused column kernels' instantiation for a fusable shape (LOGN1 in 1..4): <LOGN1, 4, 6, false>, or an EXACT one for N = 8192 with
// the reference's own parameter sets.  Returns whether it is an EXACT one; with `run`, launch(BehzColsForm<...>()) first.
template <int L1, int ML_, int MB_, bool EXACT_> struct BehzColsForm {
    static constexpr int logn1 = L1, ML = ML_, MB = MB_;
    static constexpr bool exact = EXACT_;
};
template <class Launch> bool behz_cols_dispatch(const KernelEnv &env, const BehzDev &bz, bool run, Launch &&launch)
{
    const bool exact = env.logn1 == 3 && bz.L == bz.nB && bz.L >= 2;
    if (!run) return exact;
    if (!exact) {
        dispatch_logn1(env.logn1, [&](auto n1) {
            if constexpr (decltype(n1)::value <= 4) launch(BehzColsForm<decltype(n1)::value, 4, 6, false>());
        });
    } else if (bz.L == 2) launch(BehzColsForm<3, 2, 2, true>());
    else if (bz.L == 3) launch(BehzColsForm<3, 3, 3, true>());
    else launch(BehzColsForm<3, 4, 4, true>());
    return exact;
}
bool launch_behz_extend_cols(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_cts, u64 *xq, u64 *xbsk)
{
    if (!behz_cols_fusable(env, bz)) throw std::logic_error("launch_behz_extend_cols: shape not covered by the fused kernel");
    const dim3 g((unsigned)(n_cts * 2 * 16)), blk(64u << env.logn1); // (LOGN1 = 4, N = 16384: 1024 threads, 8 KiB of LDS per residue)
    const size_t lds = behz_cols_lds_bytes(env, bz);
    return behz_cols_dispatch(env, bz, n_cts != 0, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((k_behz_extend_cols<F::logn1, F::ML, F::MB, F::exact>), g, blk, lds, env.stream, bz, env.primes, src, xq, xbsk);
    });
}
bool launch_behz_cols_floor_sk(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *dq, const u64 *ds, u64 *out)
{
    if (!behz_cols_fusable(env, bz)) throw std::logic_error("launch_behz_cols_floor_sk: shape not covered by the fused kernel");
    const dim3 g((unsigned)(n_ops * 3 * 16)), blk(64u << env.logn1);
    const size_t lds = behz_cols_lds_bytes(env, bz);
    return behz_cols_dispatch(env, bz, n_ops != 0, [&](auto f) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((k_behz_cols_floor_sk<F::logn1, F::ML, F::MB, F::exact>), g, blk, lds, env.stream, bz, env.primes, dq, ds, out);
    });
}
// the residues of both bases one engine owns: base, index in it, device prime (BehzRowsArgs, BehzTensorArgs)
template <class Args> void behz_residues(const KernelEnv &env, const BehzDev &bz, bool f64, Args &A)
{
    const auto prime_of = [&](int i) { return i < bz.L ? i : (int)bz.bsk_prime[i - bz.L]; };
    const IndexList l = engine_list(env.prime_f64, f64, bz.L + bz.nB + 1, prime_of);
    A.n_r = l.n;
    for (int k = 0; k < l.n; ++k) {
        const int i = l.at[k], base = i < bz.L ? 0 : 1;
        A.r_base[k] = (unsigned char)base; A.r_idx[k] = (unsigned char)(base ? i - bz.L : i); A.r_prime[k] = (unsigned char)prime_of(i);
    }
}
bool launch_behz_rows_tensor(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *xq, const u64 *xbsk, u64 *dq, u64 *ds)
{
    if (!n_ops) return false;
    BehzRowsArgs AE[2];
    unsigned ge[2] = {0, 0};
    const int S = bz.nB + 1;
    for (int pass = 0; pass < 2; ++pass) { // pass 0: fp64-engine residues of both bases, pass 1: u64-engine residues
        BehzRowsArgs &A = AE[pass];
        A.x[0] = xq; A.x[1] = xbsk; A.d[0] = dq; A.d[1] = ds; A.Lx[0] = bz.L; A.Lx[1] = S;
        A.n_ops = n_ops; A.logn1 = env.logn1;
        behz_residues(env, bz, pass == 0, A);
        ge[pass] = (unsigned)((n_ops * A.n_r) << env.logn1);
    }
    if (ge[0] && ge[1] && ge[0] + ge[1] <= kDualMaxBlocks) {
        hipLaunchKernelGGL(k_behz_rows_tensor_dual, dim3(ge[0] + ge[1]), dim3(kBlock), 0, env.stream, AE[0], AE[1], ge[0], env.primes);
        return true;
    }
    if (ge[0]) hipLaunchKernelGGL(k_behz_rows_tensor<ArF64>, dim3(ge[0]), dim3(kBlock), 0, env.stream, AE[0], env.primes);
    if (ge[1]) hipLaunchKernelGGL(k_behz_rows_tensor<ArU64>, dim3(ge[1]), dim3(kBlock), 0, env.stream, AE[1], env.primes);
    return false;
}
bool launch_behz_tensor_inv(const KernelEnv &env, const BehzDev &bz, const BehzSrc &src, u64 n_ops, u64 op_offset, const u64 *eq, const u64 *ebsk, u64 *dq,
                            u64 *ds)
{
    if (!n_ops) return false;
    BehzTensorArgs AE[2];
    u64 jobs[2] = {0, 0};
    const int S = bz.nB + 1;
    for (int pass = 0; pass < 2; ++pass) { // pass 0: fp64-engine residues of both bases, pass 1: u64-engine residues
        BehzTensorArgs &A = AE[pass];
        A.e[0] = eq; A.e[1] = ebsk; A.d[0] = dq; A.d[1] = ds; A.Lx[0] = bz.L; A.Lx[1] = S;
        A.src = src; A.n_ops = n_ops; A.op_offset = op_offset; A.logn1 = env.logn1;
        behz_residues(env, bz, pass == 0, A);
        jobs[pass] = ((n_ops * A.n_r) << env.logn1) * 3;
    }
    const unsigned g0 = blocks_for(jobs[0], kWaves), g1 = blocks_for(jobs[1], kWaves);
    if (jobs[0] && jobs[1] && g0 + g1 <= kDualMaxBlocks) {
        hipLaunchKernelGGL(k_behz_tensor_inv_dual, dim3(g0 + g1), dim3(kBlock), 0, env.stream, AE[0], AE[1], jobs[0], jobs[1], g0, env.primes);
        return true;
    }
    if (jobs[0]) hipLaunchKernelGGL(k_behz_tensor_inv<ArF64>, dim3(g0), dim3(kBlock), 0, env.stream, AE[0], env.primes, jobs[0]);
    if (jobs[1]) hipLaunchKernelGGL(k_behz_tensor_inv<ArU64>, dim3(g1), dim3(kBlock), 0, env.stream, AE[1], env.primes, jobs[1]);
    return false;
}
bool launch_behz_floor_sk(const KernelEnv &env, const BehzDev &bz, u64 n_ops, const u64 *dq, const u64 *ds, u64 *out)
{
    const bool wide = !(bz.L <= 4 && bz.nB <= 6);
    if (!n_ops) return wide;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_ops * 3) << logN;
    if (!wide)
        hipLaunchKernelGGL((k_behz_floor_sk<4, 6>), dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, bz, env.primes, dq, ds, out, n_ops * 3, logN);
    else
        hipLaunchKernelGGL((k_behz_floor_sk<kBehzMaxL, kBehzMaxB>), dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, bz, env.primes, dq, ds, out, n_ops * 3, logN);
    return wide;
}
void launch_bfv_galois(const KernelEnv &env, int L, u64 n_ops, const u64 *in, const uint32_t *gather, u64 *c01, u64 c01_item_stride, u64 *tgt,
                       const u64 *addend)
{
    if (!n_ops) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_ops * L) << logN;
    hipLaunchKernelGGL(k_bfv_galois, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, in, gather, c01, c01_item_stride, tgt, env.primes, L, logN,
                       n_ops, addend);
}
void launch_bfv_tail_sp(const KernelEnv &env, u64 n_polys, const u64 *tpr, u64 *rp)
{
    if (!n_polys) return;
    const unsigned g = (unsigned)(n_polys * 4);
    const int sp = env.K - 1;
    dispatch_logn1<0>(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_bfv_tail_sp<decltype(n1)::value>, dim3(g), dim3(kBlock), 0, env.stream, tpr, rp, env.primes, sp); });
}
void launch_bfv_tail_fin(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *rp, u64 *c01, u64 c01_item_stride, const u64 *add01,
                         u64 add01_item_stride)
{
    if (!add01) { add01 = c01; add01_item_stride = c01_item_stride; }
    if (!n_ops) return;
    const unsigned g = (unsigned)(n_ops * 2 * L * 4);
    dispatch_logn1<0>(env.logn1, [&](auto n1) {
        hipLaunchKernelGGL(k_bfv_tail_fin<decltype(n1)::value>, dim3(g), dim3(kBlock), 0, env.stream, t, rp, c01, c01_item_stride, add01, add01_item_stride, env.primes,
                           env.floor_consts, L, env.K);
    });
}

} // namespace HE355_KNS
} // namespace he355
